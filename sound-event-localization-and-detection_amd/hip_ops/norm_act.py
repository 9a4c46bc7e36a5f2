"""BatchNorm + activation and the gate (csrc/norm.hip), activations, pooling, dropout and transposes
(csrc/elementwise.hip), and the optimiser's gradient slots as the backward kernels' targets, with the stacked / reshaped
convolution weights that point at them."""
import os

import torch

from .. import _lib as L
from ._core import _req


# ======================================================================================
# BatchNorm + activation
# ======================================================================================
def _ncs(x):
    N, C = x.shape[0], x.shape[1]
    S = 1
    for d in x.shape[2:]:
        S *= d
    return N, C, S


STATS_REPLICAS = 64      # SELD_STATS_REPLICAS


_stats_pool = {}     # (C, device, stream) -> zero-filled statistics buffers ready for reuse


def new_stats(C, device):
    """Zeroed BatchNorm statistics buffer: SELD_STATS_REPLICAS rows of [sum(C) | sum of squares(C)].  Buffers are
    pooled: `bn_prepare` hands one back after `seld_bn_finalize_ex` has consumed AND re-zeroed it, so a training step
    does not launch a fill per BatchNorm."""
    free = _stats_pool.get((C, device, torch.cuda.current_stream(device).cuda_stream))
    if free:
        return free.pop()
    t = torch.zeros(STATS_REPLICAS * 2 * C, device=device, dtype=torch.float32)
    t._seld_pooled = True
    return t


def channel_stats(x, out=None):
    N, C, S = _ncs(x)
    stats = out if out is not None else new_stats(C, x.device)
    L.check(L.lib().seld_channel_stats(L.ptr(x), N, C, S, L.ptr(stats), L.current_stream()), "seld_channel_stats")
    return stats


def bn_prepare(x, running_mean, running_var, training, momentum, eps, stats=None, num_batches_tracked=None):
    """mean / invstd used by the normalisation; in training mode also the running-buffer update and the
    num_batches_tracked increment of torch.nn.BatchNorm, all in one launch."""
    N, C, S = _ncs(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    invstd = torch.empty(C, device=x.device, dtype=torch.float32)
    if training:
        if stats is None:
            stats = channel_stats(x)
        pooled = getattr(stats, "_seld_pooled", False)
        L.check(L.lib().seld_bn_finalize_ex(L.ptr(stats), C, N * S, eps, momentum, L.ptr(mean), L.ptr(invstd),
                                            L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked),
                                            int(pooled), L.current_stream()), "seld_bn_finalize_ex")
        if pooled:      # per stream: the buffer is re-zeroed by a kernel on THIS stream and may only be reused in order behind it
            _stats_pool.setdefault((C, x.device, torch.cuda.current_stream(x.device).cuda_stream), []).append(stats)
    else:
        L.check(L.lib().seld_bn_eval_stats(L.ptr(running_mean), L.ptr(running_var), C, eps, L.ptr(mean), L.ptr(invstd),
                                           L.current_stream()), "seld_bn_eval_stats")
    return mean, invstd


def _nbt(bn):
    """The module's num_batches_tracked buffer when torch.nn.BatchNorm would increment it, else None."""
    if bn.training and getattr(bn, "track_running_stats", True) and bn.num_batches_tracked is not None:
        return bn.num_batches_tracked
    return None


def _claim_grad_slots(params, adjacent=True):
    """Gradient slots of `params` as reduction targets.  Returns (first_slot, clean):
    first_slot -- `.grad` of the first parameter when every parameter opted in (`_seld_direct_grad`, FlatAdam) and,
                  if `adjacent`, the slots follow one another in the flat gradient buffer in this order; else None;
    clean      -- nothing has been written to the slots since the owner's last zero_grad(): the backward kernels may
                  then use the slots themselves as their (zero-initialised) output / reduction buffers.
    Marks the slots written."""
    ts = list(params)
    if not all(getattr(t, "_seld_direct_grad", False) and t.grad is not None for t in ts):
        return None, False
    if adjacent:
        at = ts[0].grad.data_ptr()
        for t in ts:
            if t.grad.data_ptr() != at:
                return None, False
            at += 4 * t.numel()
    owner = getattr(ts[0], "_seld_owner", None)
    gen = owner.grad_generation if owner is not None else None
    clean = gen is not None and all(getattr(t, "_seld_owner", None) is owner and
                                    getattr(t, "_seld_written", None) != gen for t in ts)
    for t in ts:
        t._seld_written = gen
    return ts[0].grad, clean


def _direct_targets(params, bias):
    """Gradient slots to accumulate into directly, or None.  A parameter opts in when its owner (FlatAdam)
    pre-attached `.grad` as a view of a flat buffer and set `_seld_direct_grad`."""
    ts = [getattr(t, "_seld_base_param", t) for t in params] + ([bias] if bias is not None else [])
    if all(getattr(t, "_seld_direct_grad", False) and t.grad is not None for t in ts):
        def slot(b, t):
            if b is t:
                return b.grad
            g = getattr(t, "_seld_grad", None)         # stacked_conv_weight: a slot that spans several parameters
            return g if g is not None else b.grad.view(t.shape)
        return [slot(b, t) for b, t in zip(ts, params)], (bias.grad if bias is not None else None)
    return None


def stacked_conv_weight(params):
    """ONE convolution weight (sum of the Cout's, Cin, k...) over parameters that lie back to back in memory -- FlatAdam
    re-homes a model's parameters into one flat buffer in registration order, so the attention's values / keys / queries
    (model.py:18-20) are three consecutive row blocks of it -- or None.  With gradients enabled the gradient slots must be
    adjacent in the same order too: the stacked weight is a fresh leaf over the same storage whose gradient the backward
    kernels write straight into those slots (`_direct_targets`), so autograd never sees the member parameters."""
    p0 = params[0]
    need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    at = p0.data_ptr()
    for p in params:
        if p.data_ptr() != at or not p.is_contiguous() or p.shape[1:] != p0.shape[1:] or p.dtype != torch.float32:
            return None
        at += 4 * p.numel()
    shape = (sum(int(p.shape[0]) for p in params),) + tuple(p0.shape[1:])
    same_buffer = lambda ts: all(t.untyped_storage().data_ptr() == ts[0].untyped_storage().data_ptr() for t in ts)
    if not same_buffer(params):                     # neighbours by accident of the allocator: not one tensor's memory
        return None
    gview = None
    if need_grad:
        if not all(getattr(p, "_seld_direct_grad", False) and p.grad is not None and p.requires_grad for p in params):
            return None
        if not same_buffer([p.grad for p in params]):
            return None
        gat = p0.grad.data_ptr()
        for p in params:
            if p.grad.data_ptr() != gat or not p.grad.is_contiguous():
                return None
            gat += 4 * p.numel()
        gview = p0.grad.as_strided(shape, p0.grad.stride())
    w = p0.detach().as_strided(shape, p0.stride())
    if need_grad:
        w.requires_grad_(True)
        w._seld_base_param = p0
        w._seld_grad = gview
    return w


def as_conv_weight(param, shape):
    """A contiguous reshape of a parameter used as a convolution weight (the attention's Linear applied as a 1x1
    convolution, model.py:46): the view remembers its parameter, so the backward kernels write that parameter's gradient
    slot directly instead of returning a tensor for autograd to add to it."""
    w = param.view(shape)
    w._seld_base_param = param
    return w


def axpy_(dst_first, src, n):
    """dst[0:n] += src[0:n] where dst_first is the first of several tensors that are adjacent in one flat buffer."""
    L.check(L.lib().seld_accumulate(L.ptr(dst_first), L.ptr(src), n, L.current_stream()), "seld_accumulate")


def _one_pass_ok(N, S, limit):
    """The one-workgroup-per-channel backward kernels (csrc/norm.hip) hold a channel's N*S values in registers."""
    return S % 4 == 0 and N * S <= limit and not os.environ.get("SELD_BN_TWO_PASS")


class BnActFn(torch.autograd.Function):
    """y = act(BatchNorm(x)); torch.nn.BatchNorm1d/2d + ReLU/Tanh of model.py:114-116, 279-280."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, act, stats, nbt, twin):
        x = _req(x, "x")
        N, C, S = _ncs(x)
        mean, invstd = bn_prepare(x, running_mean, running_var, training, momentum, eps, stats, nbt)
        y = torch.empty_like(x)
        L.check(L.lib().seld_bn_act_fwd(L.ptr(x), N, C, S, L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta),
                                        act, L.ptr(y), L.current_stream()), "seld_bn_act_fwd")
        ctx.training, ctx.act = training, act
        ctx.bn_params = (gamma, beta)
        ctx.save_for_backward(x, y, mean, invstd)
        ctx.twin = twin
        if twin:
            # the same values twice: each consumer's gradient then arrives separately and backward adds them while
            # it loads them (the autograd engine would launch an add kernel for a tensor used twice)
            ctx.set_materialize_grads(False)
            return y, y.view_as(y)
        return y

    @staticmethod
    def backward(ctx, dy, dy2=None):
        x, y, mean, invstd = ctx.saved_tensors
        gamma, beta = ctx.bn_params
        if dy is None:
            dy, dy2 = dy2, None
        if dy is None:
            return (None,) * 12
        dy = _req(dy, "dy")
        dy2 = _req(dy2, "dy2") if dy2 is not None else None
        none = (None,) * 9
        N, C, S = _ncs(x)
        slot, clean = _claim_grad_slots((gamma, beta))
        st = L.current_stream()
        if ctx.training and _one_pass_ok(N, S, L.SELD_BN_ONE_PASS_MAX):
            # one workgroup per channel: reads every operand once and ADDS [dgamma | dbeta] to `red`
            red = slot if slot is not None else torch.zeros(2 * C, device=x.device, dtype=torch.float32)
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            L.check(L.lib().seld_bn_act_bwd_fused(L.ptr(dy), L.ptr(x), L.ptr(y), N, C, S, L.ptr(mean), L.ptr(invstd),
                                                  L.ptr(gamma), ctx.act, L.ptr(red), L.ptr(dy2), L.ptr(dx), st),
                    "seld_bn_act_bwd_fused")
            if slot is not None:
                return (dx, None, None) + none
            return (dx, red[:C], red[C:]) + none
        if dy2 is not None:
            dy = dy + dy2
        # [dgamma | dbeta]: reduced straight into the (still zero) flat-gradient slots when possible
        red = slot if clean else torch.zeros(2 * C, device=x.device, dtype=torch.float32)
        L.check(L.lib().seld_bn_act_bwd_reduce(L.ptr(dy), L.ptr(x), L.ptr(y), N, C, S, L.ptr(mean), L.ptr(invstd),
                                               L.ptr(gamma), L.ptr(beta), ctx.act, L.ptr(red), st),
                "seld_bn_act_bwd_reduce")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.check(L.lib().seld_bn_act_bwd_apply(L.ptr(dy), L.ptr(x), L.ptr(y), N, C, S, L.ptr(mean), L.ptr(invstd),
                                                  L.ptr(gamma), L.ptr(beta), ctx.act, L.ptr(red), int(ctx.training),
                                                  L.ptr(dx), st), "seld_bn_act_bwd_apply")
        if slot is not None:
            if not clean:
                axpy_(slot, red, 2 * C)
            return (dx, None, None) + none
        return (dx, red[:C], red[C:]) + none


def bn_act(x, bn, act, stats=None, twin=False):
    """`bn` is a torch.nn.BatchNorm*-shaped module (weight, bias, running_mean, running_var, ...).  twin=True returns
    the result twice (two tensors, one storage) for a result with two consumers: see BnActFn.forward."""
    return BnActFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training,
                         bn.momentum if bn.momentum is not None else 0.1, bn.eps, act, stats, _nbt(bn), twin)


class GateFn(torch.autograd.Function):
    """y = tanh(BN_f(yf)) * sigmoid(BN_g(yg)) * channel_mask  (model.py:121-128)."""

    @staticmethod
    def forward(ctx, yf, yg, gf, bf, rmf, rvf, gg, bg, rmg, rvg, training, momentum, eps, mask, nbt_f, nbt_g,
                stats_f=None, stats_g=None):
        yf, yg = _req(yf, "yf"), _req(yg, "yg")
        N, C, S = _ncs(yf)
        if (training and stats_f is not None and stats_g is not None and getattr(stats_f, "_seld_pooled", False)
                and getattr(stats_g, "_seld_pooled", False)):
            # both layers' statistics are ready (the pair convolution gathered them): one finalize launch for the two
            mf, isf, mg, isg = (torch.empty(C, device=yf.device, dtype=torch.float32) for _ in range(4))
            L.check(L.lib().seld_bn_finalize2_ex(L.ptr(stats_f), L.ptr(stats_g), C, N * S, eps, momentum, L.ptr(mf),
                                                 L.ptr(isf), L.ptr(rmf), L.ptr(rvf), L.ptr(nbt_f), L.ptr(mg),
                                                 L.ptr(isg), L.ptr(rmg), L.ptr(rvg), L.ptr(nbt_g), 1,
                                                 L.current_stream()), "seld_bn_finalize2_ex")
            key = (C, yf.device, torch.cuda.current_stream(yf.device).cuda_stream)
            _stats_pool.setdefault(key, []).extend((stats_f, stats_g))
        else:
            mf, isf = bn_prepare(yf, rmf, rvf, training, momentum, eps, stats_f, nbt_f)
            mg, isg = bn_prepare(yg, rmg, rvg, training, momentum, eps, stats_g, nbt_g)
        y = torch.empty_like(yf)
        L.check(L.lib().seld_gate_fwd(L.ptr(yf), L.ptr(yg), N, C, S, L.ptr(mf), L.ptr(isf), L.ptr(gf), L.ptr(bf),
                                      L.ptr(mg), L.ptr(isg), L.ptr(gg), L.ptr(bg), L.ptr(mask), L.ptr(y),
                                      L.current_stream()), "seld_gate_fwd")
        ctx.training = training
        ctx.has_mask = mask is not None
        ctx.bn_params = (gf, bf, gg, bg)
        ctx.save_for_backward(yf, yg, mf, isf, mg, isg, *([mask] if mask is not None else []))
        return y

    @staticmethod
    def backward(ctx, dy):
        yf, yg, mf, isf, mg, isg, *rest = ctx.saved_tensors
        gf, bf, gg, bg = ctx.bn_params
        mask = rest[0] if ctx.has_mask else None
        dy = _req(dy, "dy")
        N, C, S = _ncs(yf)
        slot, clean = _claim_grad_slots((gf, bf, gg, bg))
        st = L.current_stream()
        if ctx.training and _one_pass_ok(N, S, L.SELD_GATE_ONE_PASS_MAX):
            red = slot if slot is not None else torch.zeros(4 * C, device=yf.device, dtype=torch.float32)
            dyf, dyg = torch.empty_like(yf), torch.empty_like(yg)
            L.check(L.lib().seld_gate_bwd_fused(L.ptr(dy), L.ptr(yf), L.ptr(yg), N, C, S, L.ptr(mf), L.ptr(isf),
                                                L.ptr(gf), L.ptr(bf), L.ptr(mg), L.ptr(isg), L.ptr(gg), L.ptr(bg),
                                                L.ptr(mask), L.ptr(red), L.ptr(dyf), L.ptr(dyg), st),
                    "seld_gate_bwd_fused")
            if slot is not None:
                return (dyf, dyg) + (None,) * 16
            return (dyf, dyg, red[:C], red[C:2 * C], None, None, red[2 * C:3 * C], red[3 * C:], None, None,
                    None, None, None, None, None, None, None, None)
        # [dgamma_f | dbeta_f | dgamma_g | dbeta_g]
        red = slot if clean else torch.zeros(4 * C, device=yf.device, dtype=torch.float32)
        args = (L.ptr(dy), L.ptr(yf), L.ptr(yg), N, C, S, L.ptr(mf), L.ptr(isf), L.ptr(gf), L.ptr(bf),
                L.ptr(mg), L.ptr(isg), L.ptr(gg), L.ptr(bg), L.ptr(mask))
        L.check(L.lib().seld_gate_bwd_reduce(*args, L.ptr(red), st), "seld_gate_bwd_reduce")
        dyf, dyg = torch.empty_like(yf), torch.empty_like(yg)
        L.check(L.lib().seld_gate_bwd_apply(*args, L.ptr(red), int(ctx.training), L.ptr(dyf), L.ptr(dyg), st),
                "seld_gate_bwd_apply")
        if slot is not None:
            if not clean:
                axpy_(slot, red, 4 * C)
            return (dyf, dyg) + (None,) * 16
        return (dyf, dyg, red[:C], red[C:2 * C], None, None, red[2 * C:3 * C], red[3 * C:], None, None,
                None, None, None, None, None, None, None, None)


def gate(yf, yg, bn_f, bn_g, mask=None, stats_f=None, stats_g=None):
    return GateFn.apply(yf, yg, bn_f.weight, bn_f.bias, bn_f.running_mean, bn_f.running_var,
                        bn_g.weight, bn_g.bias, bn_g.running_mean, bn_g.running_var, bn_f.training,
                        bn_f.momentum if bn_f.momentum is not None else 0.1, bn_f.eps, mask, _nbt(bn_f), _nbt(bn_g),
                        stats_f, stats_g)


# ======================================================================================
# activations, pooling, dropout, transposes
# ======================================================================================
class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        x = _req(x, "x")
        y = torch.empty_like(x)
        L.check(L.lib().seld_act_fwd(L.ptr(x), x.numel(), act, L.ptr(y), L.current_stream()), "seld_act_fwd")
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _req(dy, "dy")
        dx = torch.empty_like(y)
        L.check(L.lib().seld_act_bwd(L.ptr(dy), L.ptr(y), y.numel(), ctx.act, L.ptr(dx),
                                     L.current_stream()), "seld_act_bwd")
        return dx, None


def act(x, kind):
    return ActFn.apply(x, kind)


class MaxPoolFn(torch.autograd.Function):
    """torch.nn.MaxPool1d / MaxPool2d with stride == window (model.py:178,192,202,281)."""

    @staticmethod
    def forward(ctx, x, ph, pw):
        x = _req(x, "x")
        if x.dim() == 3:
            N, C, H, W = x.shape[0], x.shape[1], 1, x.shape[2]
            oshape = (N, C, W // pw)
        else:
            N, C, H, W = x.shape
            oshape = (N, C, H // ph, W // pw)
        y = torch.empty(oshape, device=x.device, dtype=torch.float32)
        idx = torch.empty(oshape, device=x.device, dtype=torch.uint8)
        L.check(L.lib().seld_maxpool_fwd(L.ptr(x), N * C, H, W, ph, pw, L.ptr(y), L.ptr(idx),
                                         L.current_stream()), "seld_maxpool_fwd")
        ctx.geom = (N * C, H, W, ph, pw, tuple(x.shape))
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        NC, H, W, ph, pw, xshape = ctx.geom
        dy = _req(dy, "dy")
        dx = torch.empty(xshape, device=dy.device, dtype=torch.float32)
        L.check(L.lib().seld_maxpool_bwd(L.ptr(dy), L.ptr(idx), NC, H, W, ph, pw, L.ptr(dx),
                                         L.current_stream()), "seld_maxpool_bwd")
        return dx, None, None


def maxpool(x, ph, pw):
    if ph == 1 and pw == 1:
        return x
    return MaxPoolFn.apply(x, int(ph), int(pw))


class _Philox:
    """Counter-based RNG bookkeeping for the dropout kernels.  The key is torch's seed (torch.manual_seed controls it)
    mixed with `stream_id` -- the data-parallel rank, so that ranks draw different masks for their different shards;
    the counter of a draw is  host offset (advances by the number of 128-bit draws) + device base.

    The device base is word 0 of the per-device STEP STATE (4 x uint64, see seld_step_begin in include/seld_hip.h):
    it is zero in eager mode; a step recorded as a HIP graph (step.GraphedTrainStep) is captured with host offsets that
    start at zero and replays with the base advanced by the draws of one step, so every replay sees fresh masks."""

    def __init__(self):
        self.offset = 0
        self.stream_id = 0
        self._state = {}

    def seed(self):
        return (torch.initial_seed() + 0x9E3779B97F4A7C15 * int(self.stream_id)) & 0xFFFFFFFFFFFFFFFF

    def state(self, device):
        """The step state tensor of `device` (int64[4], uint64 semantics): [philox base, step, lr bits, draws/step]."""
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._state.get(device)
        if t is None:
            t = self._state[device] = torch.zeros(4, device=device, dtype=torch.int64)
        return t

    def draw(self, n_groups, device):
        """(seed, offset, step-state tensor) for a kernel that consumes `n_groups` 128-bit draws."""
        off = self.offset
        self.offset += int(n_groups)
        return self.seed(), off, self.state(device)

    def get_offset(self):
        """Absolute position in the stream (checkpointed by checkpoint.save_model): host offset + device base."""
        base = sum(int(t[0].item()) for t in self._state.values())
        return self.offset + base

    def set_offset(self, offset):
        self.offset = int(offset)
        for t in self._state.values():
            t[0] = 0


philox = _Philox()


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = _req(x, "x")
        n = x.numel()
        seed, off, state = philox.draw((n + 3) // 4, x.device)
        y = torch.empty_like(x)
        L.check(L.lib().seld_dropout_fwd(L.ptr(x), n, p, seed, off, L.ptr(state), L.ptr(y), L.current_stream()),
                "seld_dropout_fwd")
        ctx.rng = (p, seed, off, state)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, off, state = ctx.rng
        dy = _req(dy, "dy")
        dx = torch.empty_like(dy)
        L.check(L.lib().seld_dropout_fwd(L.ptr(dy), dy.numel(), p, seed, off, L.ptr(state), L.ptr(dx),
                                         L.current_stream()), "seld_dropout_fwd")
        return dx, None


def dropout(x, p, training):
    if not training or p == 0.0:
        return x
    return DropoutFn.apply(x, float(p))


def channel_dropout_mask(N, C, p, device):
    """Dropout1d decision per (n, c) row, already scaled by 1/(1-p) (model.py:96-97,127-128)."""
    rows = N * C
    seed, off, state = philox.draw((rows + 3) // 4, device)
    mask = torch.empty(rows, device=device, dtype=torch.float32)
    L.check(L.lib().seld_dropout_mask_rows(rows, p, seed, off, L.ptr(state), L.ptr(mask), L.current_stream()),
            "seld_dropout_mask_rows")
    return mask


class RowScaleFn(torch.autograd.Function):
    """y[n, c, :] = x[n, c, :] * mask[n*C + c]  (stand-alone Dropout1d; inside ResBlock the mask rides in the gate kernel)."""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return _rowscale(x, mask)

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return _rowscale(_req(dy, "dy"), mask), None


def _rowscale(x, mask):
    # gate kernel with neutral BN constants would be overkill; use bn_act_fwd with gamma = mask per (n,c):
    # treat (N, C, S) as (1, N*C, S) with mean 0, invstd 1, gamma = mask, beta = 0
    x = _req(x, "x")
    N, C, S = _ncs(x)
    zeros = torch.zeros(N * C, device=x.device, dtype=torch.float32)
    ones = torch.ones(N * C, device=x.device, dtype=torch.float32)
    y = torch.empty_like(x)
    L.check(L.lib().seld_bn_act_fwd(L.ptr(x), 1, N * C, S, L.ptr(zeros), L.ptr(ones), L.ptr(mask), L.ptr(zeros),
                                    L.SELD_ACT_NONE, L.ptr(y), L.current_stream()), "seld_bn_act_fwd")
    return y


class TransposeFn(torch.autograd.Function):
    """(N, A, B) -> (N, B, A) contiguous."""

    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        N, A, B = x.shape
        y = torch.empty((N, B, A), device=x.device, dtype=torch.float32)
        L.check(L.lib().seld_transpose_nct_ntc(L.ptr(x), N, A, B, L.ptr(y), L.current_stream()), "seld_transpose")
        return y

    @staticmethod
    def backward(ctx, dy):
        return TransposeFn.apply(dy)


def transpose12(x):
    return TransposeFn.apply(x)


_identity_cache = {}


def gate_plain(yf, yg, mask=None):
    """tanh(yf) * sigmoid(yg) * mask for batch_norm='noBN' models: the gate kernel with identity
    normalisation constants (mean 0, invstd 1, gamma 1, beta 0) and eval-mode backward."""
    C = yf.shape[1]
    key = (yf.device, C)
    if key not in _identity_cache:
        _identity_cache[key] = (torch.zeros(C, device=yf.device), torch.ones(C, device=yf.device))
    zero, one = _identity_cache[key]

    return GateFn.apply(yf, yg, one, zero, zero, one, one, zero, zero, one, False, 0.1, 0.0, mask, None, None, None, None)
