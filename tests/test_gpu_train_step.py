"""The four kernels every training step ends in (csrc/train_step.hip: loss_kernel, adam_kernel, adam_state_kernel,
step_begin_kernel), element by element against fp64 expressions written here.

Both sides start from the same fp32 inputs and the same fp32-rounded hyper-parameters, so only the kernel's arithmetic
rounding separates them.  With u = 2^-24 (half an fp32 ulp) and g' = g * grad_scale + weight_decay * p:

  Adam   |m - m_ref| <= 4u (|b1 m0| + |(1 - b1) g'|)
         |v - v_ref| <= 6u (b2 v0 + (1 - b2) g'^2)
         |p - p_ref| <= tol(step) U + u |p_ref|,   U = (lr / bc1) (|b1 m0| + |(1 - b1) g'|) / denom_ref,
                                                   tol(step) = u (12 + 4 / bc1 + 2 / bc2),  bc = 1 - beta^step
         (about a dozen fp32 operations; powf within 2 ulp, amplified by the cancellation in 1 - beta^step:
         1.2e-4 at step 1, 6e-5 at step 2, below 2e-6 from step 1000 on.)  No credit for cancellation: the bounds are
         componentwise and scale with the magnitudes of the terms, not with their sum.
  loss   |dsed - ref| <= 8u |ref|,  ref = w inv (s - t) / max(s (1 - s), 1e-12)      (7 roundings)
         |ddoa - ref| <= 4u |ref|,  ref = w inv 2 (d - t)                            (4 roundings)
         both with an absolute floor of one fp32 denormal; no element is excluded, floor-dominated ones included.
         |loss - ref| <= 1e-5 max(1, |ref|), ref = fp64 BCE with the logs clamped at -100, plus the MSE.

Largest error / bound seen on the MI355X (printed by the tests; a ratio above 1 is a defect, not a reason to widen):

  Adam variant        p      m      v      update budget used, by step (1, 2, 10, 1000, 100000)
  default             0.952  0.474  0.396  0.001  0.058  0.025  0.194  0.137
  eps=1e-3            0.921  0.474  0.396  0.001  0.058  0.021  0.165  0.132
  wd=1e-2             0.979  0.625  0.640  0.000  0.046  0.002  0.000  0.000
  gs=0.25             0.897  0.466  0.410  0.001  0.058  0.023  0.165  0.157
  gs=0.25,wd=1e-2     0.981  0.604  0.642  0.000  0.047  0.000  0.000  0.000
  lr=1e-7             0.986  0.474  0.396  0.000  0.044  0.003  0.000  0.000

  loss case           dsed   ddoa   loss        loss case            dsed   ddoa   loss
  1x42x126   w1,5     0.202  0.347  0.006       1x42x126   w0.5,2    0.202  0.468  0.003
  7x3x9      w1,5     0.208  0.356  0.007       7x3x9      w0.5,2    0.208  0.448  0.004
  33x42x126  w1,5     0.271  0.371  0.003       33x42x126  w0.5,2    0.271  0.325  0.008
  600x42x126 w1,5     0.419  0.306  0.008       600x42x126 w0.5,2    0.419  0.365  0.006
  33x42x126  w1,5 soft 0.323 0.375  0.000

The p column is near 1 by construction: the bound's second term, u |p_ref|, is the rounding of p itself, and an element
just above a power of two uses all of it.  "Update budget used" is (error - u |p_ref|) / (tol(step) U) where positive:
what the update's arithmetic takes of its own allowance.  It is 0.001 at step 1, where tol is dominated by the 2 ulp
allowed to powf and powf(b, 1) is exact, and at most 0.19 elsewhere; with p ~ N(0,1) (the weight-decay variants) or
lr = 1e-7 the update is below the rounding of p and the m / v columns carry the check.  No bound is looser than 10x
everywhere, so none was tightened; none had to be widened.

The weight-decay variants found one defect: the kernels formed g' as two roundings (g * grad_scale + wd * p, compiled
to a packed multiply and an add), and where the two terms cancel the error of m, up to u |wd p| (1 - b1), was 1.5 to
7.4 times its bound on the MI355X (both weight-decay variants failed).  g' is now fma(wd, p, g * grad_scale), one rounding; with
grad_scale a power of two, as data-parallel averaging over 2^k ranks gives, the product is exact too.  Nothing changes
for weight_decay = 0, which is what training uses.
"""
import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests.helpers import pkg

gpu = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
DENORM = 2.0 ** -149
SENTINEL = -1234.5


def f32(x):
    """The value the C ABI receives for a `float` argument."""
    return float(np.float32(x))


B1, B2 = f32(0.9), f32(0.999)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(x, extra=4):
    """x on the device, followed by `extra` sentinel elements: (view of the first x.numel(), whole buffer)."""
    buf = torch.full((x.numel() + extra,), SENTINEL, dtype=x.dtype)
    buf[:x.numel()] = x.reshape(-1)
    buf = buf.to(DEV)
    return buf[:x.numel()], buf


def _guards_intact(buf, n):
    return torch.equal(_bits(buf[n:]), _bits(torch.full((buf.numel() - n,), SENTINEL)))


def _ratio(err, bound):
    """err / bound, elementwise; 0 where both are 0, inf where only the bound is."""
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


# ======================================================================================================================
# Adam
# ======================================================================================================================
ADAM_NS = (1, 255, 256, 257, 4099)
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_VARIANTS = {
    "default": dict(),
    "eps=1e-3": dict(eps=1e-3),
    "wd=1e-2": dict(wd=1e-2),
    "gs=0.25": dict(gs=0.25),
    "gs=0.25,wd=1e-2": dict(gs=0.25, wd=1e-2),
    "lr=1e-7": dict(lr=1e-4 * 0.1 ** 3),          # StepLR after three decays
}


def adam_hyper(lr=1e-4, eps=1e-8, wd=0.0, gs=1.0):
    return dict(lr=f32(lr), eps=f32(eps), wd=f32(wd), gs=f32(gs))


def adam_inputs(n, step, wd, seed):
    """fp32 (p, g, m, v).  g = N(0,1) 10^k, k in -12..3 (eps-dominated to large, g^2 finite in fp32), ~5 % exact zeros.
    Step 1 starts from zero moments; later steps from m ~ 1e-3 N(0,1), v ~ 1e-6 U(0,1), except that every second
    zero-gradient element keeps zero moments (the exact no-op).  p ~ N(0,1) with weight decay, else 1e-3 N(0,1) so that
    the rounding of p itself does not hide the update."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(-12, 4, (n,), generator=gen)
    g = torch.randn(n, generator=gen) * (10.0 ** k.double()).float()
    zero = torch.rand(n, generator=gen) < 0.05
    if n >= 255:
        zero[3], zero[n - 1] = True, True
    g[zero] = 0.0
    p = torch.randn(n, generator=gen) * (1.0 if wd else 1e-3)
    m = torch.randn(n, generator=gen) * 1e-3
    v = torch.rand(n, generator=gen) * 1e-6
    if step == 1:
        m.zero_()
        v.zero_()
    else:
        idle = zero & (torch.arange(n) % 2 == 1)
        m[idle] = 0.0
        v[idle] = 0.0
    return p, g, m, v


def adam_reference(p, g, m, v, step, lr, eps, wd, gs):
    """fp64 (p, m, v) after the step and the three componentwise bounds of the module docstring."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    pr, mr, vr = O.adam_step(p, g, m, v, step, lr=lr, b1=B1, b2=B2, eps=eps, weight_decay=wd, grad_scale=gs)
    gp = g * gs + wd * p
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    mag = (B1 * m).abs() + ((1.0 - B1) * gp).abs()
    bound_m = 4 * U * mag
    bound_v = 6 * U * (B2 * v + (1.0 - B2) * gp * gp)
    denom = (vr / bc2).sqrt() + eps
    tol = U * (12.0 + 4.0 / bc1 + 2.0 / bc2)
    bound_p = tol * (lr / bc1) * mag / denom + U * pr.abs()
    return (pr, mr, vr), (bound_p, bound_m, bound_v), tol * (lr / bc1) * mag / denom


def adam_check(inputs, got, step, hyper, what):
    """Asserts the bounds and the exact no-op of idle elements.  Returns the largest error / bound of (p, m, v) and, as
    a fourth figure, how much of the update's own budget tol(step) U was used: the bound on p is mostly the rounding of
    p itself (u |p_ref|, which an element just above a power of two uses up), so the first figure sits near 1 whatever
    the update does; the fourth is (error - u |p_ref|) / (tol(step) U) where that is positive."""
    p0, g0, m0, v0 = inputs
    refs, bounds, budget = adam_reference(p0, g0, m0, v0, step, **hyper)
    worst = []
    for name, x, r, b in zip("pmv", got, refs, bounds):
        ratio = _ratio((x.double() - r).abs(), b)
        i = int(ratio.argmax())
        worst.append(float(ratio[i]))
        assert ratio[i] <= 1.0, (f"{what}: {name}[{i}] = {float(x[i])!r}, fp64 reference {float(r[i])!r}, error / bound = "
                                 f"{float(ratio[i]):.3f} (p0 {float(p0[i])!r} g {float(g0[i])!r} m0 {float(m0[i])!r} "
                                 f"v0 {float(v0[i])!r})")
    worst.append(float(_ratio(((got[0].double() - refs[0]).abs() - U * refs[0].abs()).clamp(min=0.0), budget).max()))
    if hyper["wd"] == 0.0:
        idle = (g0 == 0) & (m0 == 0) & (v0 == 0)
        for name, x, x0 in zip("pmv", got, (p0, m0, v0)):
            assert torch.equal(_bits(x[idle]), _bits(x0[idle])), f"{what}: zero gradient, zero moments moved {name}"
    return worst


def adam_run(inputs, launch):
    """Upload (p, g, m, v) with guard elements, call launch(p, g, m, v) on the views, return the CPU results."""
    views, bufs = zip(*(_guarded(t) for t in inputs))
    launch(*views)
    torch.cuda.synchronize()
    n = inputs[0].numel()
    for name, buf in zip(("p", "g", "m", "v"), bufs):
        assert _guards_intact(buf, n), f"{name}: the elements behind the buffer were written (n = {n})"
    assert torch.equal(_bits(views[1]), _bits(inputs[1])), "the gradient buffer was written"
    return tuple(views[i].cpu() for i in (0, 2, 3))


@gpu
@pytest.mark.parametrize("variant", list(ADAM_VARIANTS))
def test_adam_flat_per_element(variant):
    H = pkg().hip_ops
    hyper = adam_hyper(**ADAM_VARIANTS[variant])
    worst = {s: [0.0] * 4 for s in ADAM_STEPS}
    for n in ADAM_NS:
        for step in ADAM_STEPS:
            inputs = adam_inputs(n, step, hyper["wd"], seed=1000 * n + step)
            got = adam_run(inputs, lambda p, g, m, v: H.adam_flat_step(
                p, g, m, v, step, lr=hyper["lr"], beta1=B1, beta2=B2, eps=hyper["eps"], weight_decay=hyper["wd"],
                grad_scale=hyper["gs"]))
            w = adam_check(inputs, got, step, hyper, f"adam[{variant}] n={n} step={step}")
            worst[step] = [max(a, b) for a, b in zip(worst[step], w)]
    print(f"\nadam[{variant}] error/bound: p {max(w[0] for w in worst.values()):.3f} | m "
          f"{max(w[1] for w in worst.values()):.3f} | v {max(w[2] for w in worst.values()):.3f} | update by step " +
          " ".join(f"{s}:{worst[s][3]:.3f}" for s in ADAM_STEPS))


def test_adam_oracle_is_torch_adam():
    """The restatement the GPU tests compare with (oracle.adam_step) is torch.optim.Adam: weight decay coupled (added to
    the gradient before the moments), eps outside the bias-corrected square root.  fp64, five steps."""
    for wd, eps, gs in ((0.0, 1e-8, 1.0), (1e-2, 1e-3, 0.25)):
        gen = torch.Generator().manual_seed(5)
        p = torch.nn.Parameter(torch.randn(64, generator=gen, dtype=torch.float64))
        opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=eps, weight_decay=wd)
        po, mo, vo = p.detach().clone(), torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
        for step in range(1, 6):
            g = torch.randn(64, generator=gen, dtype=torch.float64) * 10.0 ** torch.randint(-6, 1, (64,), generator=gen)
            p.grad = g * gs
            opt.step()
            po, mo, vo = O.adam_step(po, g, mo, vo, step, lr=1e-3, eps=eps, weight_decay=wd, grad_scale=gs)
            st = opt.state[p]
            for name, a, b in (("p", p.detach(), po), ("m", st["exp_avg"], mo), ("v", st["exp_avg_sq"], vo)):
                assert torch.all((a - b).abs() <= 1e-13 * b.abs()), (wd, eps, gs, step, name, (a - b).abs().max())
        if wd == 0.0 and gs == 1.0:       # the defaults keep the five-argument behaviour
            q = O.adam_step(po, g, mo, vo, 6)
            r = O.adam_step(po, g, mo, vo, 6, weight_decay=0.0, grad_scale=1.0)
            assert all(torch.equal(a, b) for a, b in zip(q, r))


# ======================================================================================================================
# step state: seld_adam_flat_state, seld_step_begin
# ======================================================================================================================
BASE, DRAWS = (1 << 32) + 5, 12345          # a Philox base past 32 bits


def _lr_bits(lr):
    return int(np.float32(lr).view(np.uint32))


def _state(step, lr, high=0):
    return torch.tensor([BASE, step, _lr_bits(lr) | (high << 32), DRAWS], dtype=torch.int64, device=DEV)


@gpu
@pytest.mark.parametrize("step", [1, 10])
@pytest.mark.parametrize("n", [257, 4099])
def test_adam_flat_state_is_adam_flat(n, step):
    """step / lr read from the device-resident state: the bits of seld_adam_flat, the Philox base moved past the step's
    draws, nothing else in the state touched; only the low word of state[2] is the learning rate."""
    H = pkg().hip_ops
    hyper = adam_hyper(lr=3e-5, wd=1e-2, gs=0.25)
    kw = dict(beta1=B1, beta2=B2, eps=hyper["eps"], weight_decay=hyper["wd"], grad_scale=hyper["gs"])
    inputs = adam_inputs(n, step, hyper["wd"], seed=77 * n + step)
    flat = adam_run(inputs, lambda p, g, m, v: H.adam_flat_step(p, g, m, v, step, lr=hyper["lr"], **kw))
    adam_check(inputs, flat, step, hyper, f"adam_flat n={n} step={step}")
    for high in (0, 0x7FC0FFEE):
        state = _state(step, hyper["lr"], high)
        got = adam_run(inputs, lambda p, g, m, v: H.adam_flat_step_state(p, g, m, v, state, **kw))
        for name, a, b in zip("pmv", got, flat):
            assert torch.equal(_bits(a), _bits(b)), f"{name} differs from seld_adam_flat (high word {high:#x})"
        assert state.tolist() == [BASE + DRAWS, step, _lr_bits(hyper["lr"]) | (high << 32), DRAWS]


@gpu
def test_adam_flat_state_without_elements_still_ends_the_step():
    """n == 0: nothing to update, but the launch is still the end of the step -- state[0] += state[3], as
    seld_step_begin(n == 0) still advances state[1]."""
    L = pkg()._lib
    bufs = [torch.full((4,), SENTINEL, device=DEV) for _ in range(4)]
    state = _state(3, 1e-4)
    rc = L.lib().seld_adam_flat_state(*(L.ptr(b) for b in bufs), 0, B1, B2, f32(1e-8), 0.0, 1.0, L.ptr(state),
                                      L.current_stream())
    torch.cuda.synchronize()
    assert rc == L.SELD_OK
    assert state.tolist() == [BASE + DRAWS, 3, _lr_bits(1e-4), DRAWS]
    for b in bufs:
        assert _guards_intact(b, 0)


STEP_BEGIN_NS = (0, 1, 3, 4, 5, 1023, 4099)


def _poisoned(n):
    buf = torch.full((n + 4,), SENTINEL)
    buf[:n] = float("nan")
    return buf.to(DEV)


@gpu
@pytest.mark.parametrize("with_state", [True, False], ids=["state", "no_state"])
@pytest.mark.parametrize("n", STEP_BEGIN_NS)
def test_step_begin(n, with_state):
    """The first n floats become +0.0 (float4 body and the n % 4 tail), nothing behind them is written, state[1]
    advances by exactly one and the other three words stay."""
    L = pkg()._lib
    buf = _poisoned(n)
    state = _state(41, 1e-4)
    rc = L.lib().seld_step_begin(L.ptr(buf), n, L.ptr(state if with_state else None), L.current_stream())
    torch.cuda.synchronize()
    assert rc == L.SELD_OK
    assert torch.equal(_bits(buf[:n]), torch.zeros(n, dtype=torch.int32))
    assert _guards_intact(buf, n)
    assert state.tolist() == [BASE, 42 if with_state else 41, _lr_bits(1e-4), DRAWS]


@gpu
def test_step_begin_through_the_wrapper():
    H = pkg().hip_ops
    buf = _poisoned(1023)
    state = _state(1, 1e-4)
    H.step_begin(buf[:1023], state)
    H.step_begin(buf[:1023])
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf[:1023]), torch.zeros(1023, dtype=torch.int32))
    assert _guards_intact(buf, 1023)
    assert state.tolist() == [BASE, 2, _lr_bits(1e-4), DRAWS]


@gpu
def test_step_begin_refuses_a_misaligned_buffer():
    """The body stores float4: a pointer that is not 16-byte aligned is an argument error, answered before any launch."""
    L = pkg()._lib
    buf = _poisoned(12)
    before = _bits(buf)
    state = _state(41, 1e-4)
    rc = L.lib().seld_step_begin(L.ptr(buf[1:]), 8, L.ptr(state), L.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and L._ERRORS[rc] == "SELD_EINVAL"
    assert torch.equal(_bits(buf), before)
    assert state.tolist() == [BASE, 41, _lr_bits(1e-4), DRAWS]


# ======================================================================================================================
# loss
# ======================================================================================================================
LOSS_SHAPES = ((1, 42, 126), (7, 3, 9), (33, 42, 126), (600, 42, 126))     # the last: grid-stride loop, 256-block cap
LOSS_CASES = [(shape, w, False) for shape in LOSS_SHAPES for w in ((1.0, 5.0), (0.5, 2.0))] + \
             [((33, 42, 126), (1.0, 5.0), True)]


def loss_inputs(rows, n_sed, n_doa, soft, seed):
    """fp32 (sed, doa, target).  sed = sigmoid of logits over +-30: ~1e-13 ... 1 - 2^-24 and exactly 1.0; the first
    elements are set by hand to 0, 1, 1e-30, 1e-9 and 1 - 2^-24 against both targets, and a denormal against t = 1.
    (Against t = 0 the smallest hand-set value is 1e-30: the kernel forms w inv (s - t) before it divides, and below
    s ~ 1e-33 that product is an fp32 denormal, so the gradient -- itself below 1e-21 -- keeps fewer bits than 8u asks.)
    Targets {0, 1}, or 0.3 everywhere (soft).  doa, its target in [-1, 1], with +-1 and an exact match set by hand."""
    gen = torch.Generator().manual_seed(seed)
    sed = torch.sigmoid(torch.rand(rows, n_sed, generator=gen) * 60 - 30)
    t_sed = (torch.rand(rows, n_sed, generator=gen) < 0.3).float()
    hand = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (DENORM, 1.0), (1 - U, 0.0), (1e-9, 1.0), (1 - U, 1.0),
            (1e-30, 0.0), (1e-9, 0.0)]
    sf, tf = sed.view(-1), t_sed.view(-1)
    for i, (s, t) in enumerate(hand[:sf.numel() // 2]):
        sf[i], tf[i] = s, t
    if soft:
        t_sed.fill_(0.3)
    doa = torch.rand(rows, n_doa, generator=gen) * 2 - 1
    t_doa = torch.rand(rows, n_doa, generator=gen) * 2 - 1
    df, tdf = doa.view(-1), t_doa.view(-1)
    df[0], tdf[0] = 1.0, -1.0
    df[1], tdf[1] = -1.0, 1.0
    tdf[2] = df[2]
    return sed, doa, torch.cat((t_sed, t_doa), 1)


def loss_reference(sed, doa, target, w_sed, w_doa):
    """fp64 from the fp32 inputs: (loss, dloss/dsed, dloss/ddoa)."""
    rows, n_sed = sed.shape
    n_doa = doa.shape[1]
    s, d, t, td = sed.double(), doa.double(), target[:, :n_sed].double(), target[:, n_sed:].double()
    inv_s, inv_d = 1.0 / (rows * n_sed), 1.0 / (rows * n_doa)
    l1, l0 = torch.log(s).clamp(min=-100.0), torch.log(1.0 - s).clamp(min=-100.0)
    loss = w_sed * inv_s * float(-(t * l1 + (1.0 - t) * l0).sum()) + w_doa * inv_d * float(((d - td) ** 2).sum())
    return loss, w_sed * inv_s * (s - t) / (s * (1.0 - s)).clamp(min=1e-12), w_doa * inv_d * 2.0 * (d - td)


_loss_refs = {}


def loss_case(shape, weights, soft):
    """Inputs and fp64 reference of a case, computed once and shared (read only)."""
    key = (shape, weights, soft)
    if key not in _loss_refs:
        inputs = loss_inputs(*shape, soft, seed=sum(shape) + int(soft))
        _loss_refs[key] = (inputs, loss_reference(*inputs, *weights))
    return _loss_refs[key]


def loss_check(got, ref, what):
    """Asserts the three bounds of the module docstring; returns the largest error / bound of (dsed, ddoa)."""
    (loss, dsed, ddoa), (loss_r, dsed_r, ddoa_r) = got, ref
    assert abs(loss - loss_r) <= 1e-5 * max(1.0, abs(loss_r)), f"{what}: loss {loss!r}, fp64 reference {loss_r!r}"
    worst = []
    for name, x, r, k in (("dsed", dsed, dsed_r, 8), ("ddoa", ddoa, ddoa_r, 4)):
        ratio = _ratio((x.double() - r).abs(), k * U * r.abs() + DENORM).view(-1)
        i = int(ratio.argmax())
        worst.append(float(ratio[i]))
        assert ratio[i] <= 1.0, (f"{what}: {name}[{i}] = {float(x.view(-1)[i])!r}, fp64 reference "
                                 f"{float(r.view(-1)[i])!r}, error / bound = {float(ratio[i]):.3f}")
    return worst


_LOSS_IDS = [f"{'x'.join(map(str, s))}-w{w[0]:g},{w[1]:g}{'-soft' if soft else ''}" for s, w, soft in LOSS_CASES]


@gpu
@pytest.mark.parametrize("shape,weights,soft", LOSS_CASES, ids=_LOSS_IDS)
def test_loss_per_element(shape, weights, soft):
    H, L = pkg().hip_ops, pkg()._lib
    (sed, doa, tgt), ref = loss_case(shape, weights, soft)
    rows, n_sed, n_doa = shape
    what = f"loss[{_LOSS_IDS[LOSS_CASES.index((shape, weights, soft))]}]"

    # through autograd, (batch, frames, channels) as the training step calls it
    a, b = sed[None].to(DEV).requires_grad_(True), doa[None].to(DEV).requires_grad_(True)
    td = tgt.to(DEV)
    loss = H.seld_loss(a, b, td[None], *weights)
    loss.backward()
    r_sed, r_doa = loss_check((loss.item(), a.grad[0].cpu(), b.grad[0].cpu()), ref, what)

    # the C ABI, with guard elements behind all three outputs: the same bits
    auto_sed, auto_doa = a.grad.reshape(-1), b.grad.reshape(-1)
    a, b = a.detach()[0], b.detach()[0]
    (lv, lbuf), (gsv, gsbuf), (gdv, gdbuf) = (_guarded(torch.full((k,), float("nan"))) for k in (1, sed.numel(), doa.numel()))
    L.check(L.lib().seld_loss_fwd_bwd(L.ptr(a), L.ptr(b), L.ptr(td), rows, n_sed, n_doa, *weights, L.ptr(lv), L.ptr(gsv),
                                      L.ptr(gdv), L.current_stream()), "seld_loss_fwd_bwd")
    # forward only: the same loss bits, and no gradient written anywhere
    (fv, fbuf) = _guarded(torch.full((1,), float("nan")))
    idle = [torch.full((k,), SENTINEL, device=DEV) for k in (sed.numel(), doa.numel())]
    L.check(L.lib().seld_loss_fwd_bwd(L.ptr(a), L.ptr(b), L.ptr(td), rows, n_sed, n_doa, *weights, L.ptr(fv), None, None,
                                      L.current_stream()), "seld_loss_fwd_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(lbuf, 1) and _guards_intact(gsbuf, sed.numel()) and _guards_intact(gdbuf, doa.numel())
    assert _guards_intact(fbuf, 1) and all(_guards_intact(t, 0) for t in idle)
    assert _bits(lv).item() == _bits(loss.reshape(1)).item() == _bits(fv).item()
    assert torch.equal(_bits(gsv), _bits(auto_sed)) and torch.equal(_bits(gdv), _bits(auto_doa))
    loss_check((lv.item(), gsv.cpu().view(rows, n_sed), gdv.cpu().view(rows, n_doa)), ref, what + " (C ABI)")
    print(f"\n{what} error/bound: dsed {r_sed:.3f} | ddoa {r_doa:.3f} | loss "
          f"{abs(loss.item() - ref[0]) / (1e-5 * max(1.0, abs(ref[0]))):.3f}")
