"""The first CNN stage fused (csrc/first_stage.hip, csrc/hcq_first.hip, csrc/norm.hip, csrc/elementwise.hip)."""
import ctypes
import os

import torch

from .. import _lib as L
from ._core import _req, deterministic, kernel_timer, memo
from .conv import (_conv_backward, _conv_forward, _timed, _y_shape, conv_fwd, conv_out_shape, hcq_label, hyper_conv,
                   make_conv_desc)
from .norm_act import _claim_grad_slots, _direct_targets, _nbt, axpy_, bn_prepare, dropout, new_stats, philox
from .streams import _side_enabled, side_queue
from .weight_forms import hcq_pack_floats, hcq_weights


# ======================================================================================
# fused CNN stage: conv (+ BatchNorm statistics in its epilogue) -> BN -> ReLU -> MaxPool
# ======================================================================================
class HyperConvStatsFn(torch.autograd.Function):
    """y = W (x) x and, from the same kernel's epilogue, the per-channel sum / sum of squares of y
    (SELD_EPI_STATS) that the BatchNorm which follows needs: saves one full read of y."""

    @staticmethod
    def forward(ctx, x, bias, stride, padding, dilation, *ws):
        x = _req(x, "x")
        stats = new_stats(ws[0].shape[0] * len(ws), x.device)
        y = _conv_forward(ctx, x, bias, ws, stride, padding, dilation, epilogue=L.SELD_EPI_STATS, stats=stats)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)        # no zero-filled "gradient" of the statistics buffer per backward pass
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        if dy is None:
            return (None,) * (5 + len(ctx.w_params))
        dx, dbias, dws = _conv_backward(ctx, dy, 5)
        return (dx, dbias, None, None, None, *dws)


def hyper_conv_stats(x, ws, bias, stride, padding, dilation):
    return HyperConvStatsFn.apply(x, bias, stride, padding, dilation, *ws)


def _draw_dropout(ctx, drop_p, like):
    """(p, seed, offset, step state) of Dropout(drop_p) on `like`, drawn as a DropoutFn would here and kept in ctx.rng for
    the backward pass; the kernels' "no dropout" arguments for drop_p == 0."""
    if drop_p <= 0.0:
        return 0.0, 0, 0, None
    ctx.rng = (float(drop_p),) + philox.draw((like.numel() + 3) // 4, like.device)
    return ctx.rng


class BnReluPoolFn(torch.autograd.Function):
    """[Dropout(drop_p)](MaxPool2d(ph, pw)(ReLU(BatchNorm2d(y)))) in one pass each way (model.py:278-282)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, training, momentum, eps, ph, pw, stats, nbt, drop_p):
        y = _req(y, "y")
        N, C, Hh, Ww = y.shape
        mean, invstd = bn_prepare(y, running_mean, running_var, training, momentum, eps, stats, nbt)
        pooled = torch.empty((N, C, Hh // ph, Ww // pw), device=y.device, dtype=torch.float32)
        idx = torch.empty(pooled.shape, device=y.device, dtype=torch.uint8)
        ctx.rng = None
        p_, seed, off, state = _draw_dropout(ctx, drop_p, pooled)
        out = torch.empty_like(pooled) if p_ > 0.0 else None
        L.check(L.lib().seld_bn_relu_pool_fwd_drop(L.ptr(y), N, C, Hh, Ww, ph, pw, L.ptr(mean), L.ptr(invstd),
                                                   L.ptr(gamma), L.ptr(beta), L.ptr(pooled), L.ptr(idx), p_, seed, off,
                                                   L.ptr(state), L.ptr(out),
                                                   L.current_stream()), "seld_bn_relu_pool_fwd_drop")
        ctx.geom = (N, C, Hh, Ww, ph, pw, training)
        ctx.bn_params = (gamma, beta)
        ctx.save_for_backward(y, pooled, idx, mean, invstd)
        return pooled if out is None else out

    @staticmethod
    def backward(ctx, dpooled):
        y, pooled, idx, mean, invstd = ctx.saved_tensors
        gamma, beta = ctx.bn_params
        N, C, Hh, Ww, ph, pw, training = ctx.geom
        dpooled = _req(dpooled, "dpooled")
        slot, clean = _claim_grad_slots((gamma, beta))
        red = slot if clean else torch.zeros(2 * C, device=y.device, dtype=torch.float32)
        dy = torch.empty_like(y)
        p_, seed, off, state = ctx.rng if ctx.rng is not None else (0.0, 0, 0, None)
        L.check(L.lib().seld_bn_relu_pool_bwd_drop(L.ptr(dpooled), L.ptr(pooled), L.ptr(idx), L.ptr(y), N, C, Hh, Ww,
                                                   ph, pw, L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta),
                                                   int(training), L.ptr(red), L.ptr(dy), p_, seed, off, L.ptr(state),
                                                   L.current_stream()),
                "seld_bn_relu_pool_bwd_drop")
        if slot is not None:
            if not clean:
                axpy_(slot, red, 2 * C)     # one add into the flat gradient slice [dgamma | dbeta]
            return (dy,) + (None,) * 12
        return (dy, red[:C], red[C:]) + (None,) * 10


def bn_relu_pool(y, bn, ph, pw, stats=None, drop_p=0.0):
    """drop_p > 0 (training): the stage's Dropout rides in the same kernels when the shape allows, else it follows."""
    drop_p = float(drop_p) if bn.training else 0.0
    fuse = drop_p > 0.0 and bool(L.lib().seld_bn_relu_pool_drop_ok(int(y.shape[2]), int(y.shape[3]), int(ph), int(pw)))
    out = BnReluPoolFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training,
                             bn.momentum if bn.momentum is not None else 0.1, bn.eps, int(ph), int(pw), stats, _nbt(bn),
                             drop_p if fuse else 0.0)
    return out if fuse or drop_p == 0.0 else dropout(out, drop_p, True)


class ConvBnReluPoolFn(torch.autograd.Function):
    """pooled = MaxPool2d(ph, 1)(ReLU(BatchNorm2d(W (x) x))) for a convolution whose INPUT needs no gradient -- the first
    CNN stage (model.py:269-283 on the network input).  Forward is the same three kernels as hyper_conv_stats +
    bn_relu_pool.  Backward never writes the gradient w.r.t. the conv output (1.6 GB at batch 32): the per-channel
    reductions come from pooled-size tensors (seld_bn_relu_pool_bwd_coef) and the weight-gradient kernel forms
    dy = y*c1 + dz*a + c0 while it stages its operand (seld_hc_conv_bwd_weight_bnpool_acc).  Needs FlatAdam's gradient
    slots (the kernel accumulates); `conv_bn_relu_pool` falls back to the two separate functions otherwise."""

    @staticmethod
    def forward(ctx, x, bias, gamma, beta, running_mean, running_var, training, momentum, eps, ph, nbt, stride, padding,
                dilation, drop_p, *ws):
        algebra = len(ws)
        ctx.rng = None
        k = tuple(ws[0].shape[2:])
        desc = make_conv_desc(tuple(x.shape), ws[0].shape[0] * algebra, algebra, k, stride, padding, dilation)
        x = _req(x, "x")
        # The step's first request for packed weight forms re-packs every registered layer (one launch, ~50 us).  The
        # input's second moments do not need them: when the no-output path is going to be taken they are gathered on the side
        # stream WHILE the main stream packs, and joined before BatchNorm is evaluated from them.
        gws = early = None
        if (ph == 8 and algebra > 1 and training and _side_enabled() and not kernel_timer.active and
                hcq_weights.repack_pending() and _first_stage_nostore(desc) and hcq_pack_floats(desc, 2) > 0):
            # (only when a re-pack is pending -- the two-stream model packs before it forks its branches; timed steps keep the
            #  stage's launches on one stream, in one bracket)
            gws = torch.empty(_fs_bytes(desc, "gram"), device=x.device, dtype=torch.uint8)
            with side_queue.fork(gws, x):
                L.check(L.lib().seld_first_stage_gram(ctypes.byref(desc), L.ptr(x), L.ptr(gws), gws.numel(),
                                                      L.current_stream()), "seld_first_stage_gram")
                early = side_queue.event()
        wp = hcq_weights.get(desc, 2, ws) if (ph == 8 and algebra > 1) else None
        if early is not None:
            torch.cuda.current_stream().wait_event(early)
        nostore = wp is not None and training and _first_stage_nostore(desc)
        stats = new_stats(desc.Cout, x.device) if training and not nostore else None
        ctx.gram = None
        if nostore:
            # no convolution output at all (csrc/first_stage.hip): BatchNorm's statistics from the input's second moments,
            # the pooling convolution writes the window value + row only, the backward pass works from those and x
            lib = L.lib()
            o = conv_out_shape(desc)
            N, C, Hh, Ww = _y_shape(desc, o)
            with _timed(desc, 0, label="first_stage_fwd(gram+bn+finishing_pool_conv)"):
                if early is None:
                    gws = torch.empty(_fs_bytes(desc, "gram"), device=x.device, dtype=torch.uint8)
                    L.check(lib.seld_first_stage_gram(ctypes.byref(desc), L.ptr(x), L.ptr(gws), gws.numel(),
                                                      L.current_stream()), "seld_first_stage_gram")
                mean = torch.empty(C, device=x.device, dtype=torch.float32)
                invstd = torch.empty(C, device=x.device, dtype=torch.float32)
                wg = torch.empty((C, 72), device=x.device, dtype=torch.float32)
                L.check(lib.seld_first_stage_bn(ctypes.byref(desc), L.ptr_array8([_req(w, "w") for w in ws]),
                                                L.ptr(_req(bias, "bias")), L.ptr(gws), eps, momentum, L.ptr(mean),
                                                L.ptr(invstd), L.ptr(running_mean), L.ptr(running_var), L.ptr(nbt),
                                                L.ptr(wg), L.current_stream()), "seld_first_stage_bn")
                # raw: written (and read by the backward pass) only for channels with gamma == 0; untouched memory otherwise
                raw = torch.empty((N, C, Hh // ph, Ww), device=x.device, dtype=torch.float32)
                idx = torch.empty(raw.shape, device=x.device, dtype=torch.uint8)
                result = torch.empty_like(raw)
                p_, seed, off, state = _draw_dropout(ctx, drop_p, raw)
                L.check(lib.seld_hcq_first_pool_bn(ctypes.byref(desc), L.ptr(x), L.ptr(wp), L.ptr(_req(bias, "bias")),
                                                   L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(invstd), p_, seed, off,
                                                   L.ptr(state), L.ptr(raw), L.ptr(idx), L.ptr(result),
                                                   L.current_stream()), "seld_hcq_first_pool_bn")
            ctx.desc, ctx.geom = desc, (N, C, Hh, Ww, ph, training)
            ctx.params = (ws, bias, gamma, beta)
            ctx.gram = (gws, wg)
            ctx.save_for_backward(x, raw, idx, mean, invstd, result)      # the output's zeros replay ReLU + Dropout backward
            return result
        if wp is not None:
            # the convolution picks every pooling window's element itself (by the sign of gamma): y is written for the
            # backward pass but never read back in the forward pass (csrc/hcq_first.hip hcq_first_pool_kernel)
            o = conv_out_shape(desc)
            y = torch.empty(_y_shape(desc, o), device=x.device, dtype=torch.float32)
            N, C, Hh, Ww = y.shape
            raw = torch.empty((N, C, Hh // ph, Ww), device=x.device, dtype=torch.float32)
            idx = torch.empty(raw.shape, device=x.device, dtype=torch.uint8)
            with _timed(desc, 0, label=lambda: hcq_label(desc, 2, 1)):
                L.check(L.lib().seld_hcq_first_pool(ctypes.byref(desc), L.ptr(x), L.ptr(wp), L.ptr(_req(bias, "bias")),
                                                    L.ptr(gamma), int(training), L.ptr(y), L.ptr(stats), L.ptr(raw),
                                                    L.ptr(idx), L.current_stream()), "seld_hcq_first_pool")
            mean, invstd = bn_prepare(y, running_mean, running_var, training, momentum, eps, stats, nbt)
            pooled = torch.empty_like(raw)
            p_, seed, off, state = _draw_dropout(ctx, drop_p, pooled)       # the stage's Dropout in the same pass
            out = torch.empty_like(raw) if p_ > 0.0 else None
            L.check(L.lib().seld_bn_pool_finish(L.ptr(raw), N, C, (Hh // ph) * Ww, L.ptr(mean), L.ptr(invstd),
                                                L.ptr(gamma), L.ptr(beta), L.ptr(pooled), p_, seed, off, L.ptr(state),
                                                L.ptr(out), L.current_stream()),
                    "seld_bn_pool_finish")
        else:
            y = conv_fwd(desc, x, ws, bias, epilogue=L.SELD_EPI_STATS if training else 0, stats=stats)
            N, C, Hh, Ww = y.shape
            mean, invstd = bn_prepare(y, running_mean, running_var, training, momentum, eps, stats, nbt)
            pooled = torch.empty((N, C, Hh // ph, Ww), device=y.device, dtype=torch.float32)
            idx = torch.empty(pooled.shape, device=y.device, dtype=torch.uint8)
            L.check(L.lib().seld_bn_relu_pool_fwd(L.ptr(y), N, C, Hh, Ww, ph, 1, L.ptr(mean), L.ptr(invstd), L.ptr(gamma),
                                                  L.ptr(beta), L.ptr(pooled), L.ptr(idx), L.current_stream()),
                    "seld_bn_relu_pool_fwd")
            out = None
            if drop_p > 0.0:
                p_, seed, off, state = _draw_dropout(ctx, drop_p, pooled)
                out = torch.empty_like(pooled)
                L.check(L.lib().seld_dropout_fwd(L.ptr(pooled), pooled.numel(), drop_p, seed, off, L.ptr(state),
                                                 L.ptr(out), L.current_stream()), "seld_dropout_fwd")
        ctx.desc, ctx.geom = desc, (N, C, Hh, Ww, ph, training)
        ctx.params = (ws, bias, gamma, beta)
        ctx.save_for_backward(x, y, pooled, idx, mean, invstd)
        return pooled if out is None else out

    @staticmethod
    def backward(ctx, dpooled):
        if ctx.gram is not None:
            return ConvBnReluPoolFn._backward_nostore(ctx, dpooled)
        x, y, pooled, idx, mean, invstd = ctx.saved_tensors
        ws, bias, gamma, beta = ctx.params
        N, C, Hh, Ww, ph, training = ctx.geom
        dpooled = _req(dpooled, "dpooled")
        # ctx.rng: `dpooled` is the gradient BEHIND the stage's Dropout; both consumers replay its mask while they load it
        p_, seed, off, state = ctx.rng if ctx.rng is not None else (0.0, 0, 0, None)
        drop = (p_, seed, off, L.ptr(state))
        direct = _direct_targets(ws, bias)
        if direct is None:
            raise L.SeldHipError("ConvBnReluPoolFn needs gradient slots (FlatAdam); use hyper_conv_stats + bn_relu_pool")
        slot, clean = _claim_grad_slots((gamma, beta))
        red = slot if clean else torch.zeros(2 * C, device=y.device, dtype=torch.float32)
        coef = torch.empty(3 * C, device=y.device, dtype=torch.float32)
        st = L.current_stream()
        L.check(L.lib().seld_bn_relu_pool_bwd_coef_drop(L.ptr(dpooled), L.ptr(pooled), L.ptr(idx), L.ptr(y), N, C, Hh, Ww, ph,
                                                        1, L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta),
                                                        int(training), L.ptr(red), L.ptr(coef), L.ptr(direct[1]), *drop, st),
                "seld_bn_relu_pool_bwd_coef_drop")
        with _timed(ctx.desc, 2, 1, True):
            L.check(L.lib().seld_hc_conv_bwd_weight_bnpool_drop_acc(ctypes.byref(ctx.desc), L.ptr(x), L.ptr(y),
                                                                    L.ptr(pooled), L.ptr(dpooled), L.ptr(idx), ph,
                                                                    L.ptr(coef), L.ptr_array8(direct[0]), *drop, st),
                    "seld_hc_conv_bwd_weight_bnpool_drop_acc")
        dg = db = None
        if slot is None:
            dg, db = red[:C], red[C:]
        elif not clean:
            axpy_(slot, red, 2 * C)
        return (None, None, dg, db) + (None,) * (11 + len(ws))


    @staticmethod
    def _backward_nostore(ctx, dout):
        x, raw, idx, mean, invstd, out = ctx.saved_tensors
        ws, bias, gamma, beta = ctx.params
        gws, wg = ctx.gram
        N, C, Hh, Ww, ph, training = ctx.geom
        dout = _req(dout, "dout")
        p_, seed, off, state = ctx.rng if ctx.rng is not None else (0.0, 0, 0, None)
        direct = _direct_targets(ws, bias)
        if direct is None:
            raise L.SeldHipError("ConvBnReluPoolFn needs gradient slots (FlatAdam); use hyper_conv_stats + bn_relu_pool")
        slot, _ = _claim_grad_slots((gamma, beta))
        red = slot if slot is not None else torch.zeros(2 * C, device=x.device, dtype=torch.float32)
        nbytes = _fs_bytes(ctx.desc, "bwd")
        wsb = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
        with _timed(ctx.desc, 2, 1, label="fs_wgrad_kernel"):
            L.check(L.lib().seld_first_stage_bwd(ctypes.byref(ctx.desc), L.ptr(x), L.ptr(dout), L.ptr(out), L.ptr(raw),
                                                 L.ptr(idx), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta),
                                                 L.ptr(bias), L.ptr(gws), L.ptr(wg), L.ptr(red),
                                                 ctypes.c_void_p(red.data_ptr() + 4 * C), L.ptr_array8(direct[0]), p_,
                                                 L.ptr(wsb), nbytes, L.current_stream()),
                    "seld_first_stage_bwd")
        dg = db = None
        if slot is None:
            dg, db = red[:C], red[C:]
        return (None, None, dg, db) + (None,) * (11 + len(ws))


@memo
def _fs_bytes(desc, which):
    """Scratch bytes of the no-output first stage (csrc/first_stage.hip) for `desc`: which = 'gram' | 'bwd'; 0 = not taken."""
    lib = L.lib()
    fn = lib.seld_first_stage_gram_workspace if which == "gram" else lib.seld_first_stage_bwd_workspace
    return int(fn(ctypes.byref(desc)))


def _first_stage_nostore(desc):
    """The first stage without its convolution output: 8 real input channels, shapes first_stage.hip takes (forward AND
    backward), SELD_FIRST_STAGE_STORE_Y=1 restores the path that writes y."""
    return (desc.Cin == 8 and not os.environ.get("SELD_FIRST_STAGE_STORE_Y") and _fs_bytes(desc, "gram") > 0 and
            _fs_bytes(desc, "bwd") > 0)


def conv_bn_relu_pool(x, ws, bias, bn, ph, pw, stride, padding, dilation, drop_p=0.0):
    """conv -> BatchNorm2d -> ReLU -> MaxPool2d(ph, pw) [-> Dropout(drop_p), training mode].  The first stage of the
    network (x needs no gradient) takes the fused forms above when the shape qualifies; everything else is
    hyper_conv[_stats] + bn_relu_pool + dropout."""
    drop_p = float(drop_p) if bn.training else 0.0
    k = tuple(ws[0].shape[2:])
    one = lambda v: v == 1 or tuple(v) == (1, 1) if isinstance(v, (tuple, list)) else v == 1
    fused = (not x.requires_grad and torch.is_grad_enabled() and x.dim() == 4 and k == (3, 3) and int(pw) == 1 and
             one(stride) and one(dilation) and x.shape[2] % int(ph) == 0 and x.shape[3] % 32 == 0 and
             _direct_targets(ws, bias) is not None and not os.environ.get("SELD_NO_FUSED_STAGE0"))
    if fused:
        pad = padding if isinstance(padding, (tuple, list)) else (padding, padding)
        fused = tuple(pad) == (1, 1)          # 'same' 3x3: the output has the input's height and width
    if fused and deterministic():
        # only the path without the convolution output is free of atomics (Gram statistics, partials + ordered folds)
        desc_ = make_conv_desc(tuple(x.shape), ws[0].shape[0] * len(ws), len(ws), k, stride, padding, dilation)
        fused = (len(ws) > 1 and int(ph) == 8 and bn.training and _first_stage_nostore(desc_) and
                 hcq_weights.get(desc_, 2, ws) is not None)
    if fused:
        return ConvBnReluPoolFn.apply(x, bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training,
                                      bn.momentum if bn.momentum is not None else 0.1, bn.eps, int(ph), _nbt(bn),
                                      stride, padding, dilation, drop_p, *ws)
    if bn.training:
        y, stats = hyper_conv_stats(x, ws, bias, stride, padding, dilation)
    else:
        y, stats = hyper_conv(x, ws, bias, stride, padding, dilation), None
    return bn_relu_pool(y, bn, ph, pw, stats, drop_p)
