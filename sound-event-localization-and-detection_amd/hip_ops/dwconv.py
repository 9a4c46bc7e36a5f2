"""Depthwise convolution (csrc/dwconv.hip): descriptor, the three entry points, autograd function."""
import ctypes

import torch

from .. import _lib as L
from ._core import _req, kernel_label, scratch, timed
from .conv import make_conv_desc
from .norm_act import _claim_grad_slots
from .train_ops import step_begin


# ---- depthwise convolution (csrc/dwconv.hip) ----------------------------------------------------------------------------
# nn.Conv1d / nn.Conv2d with groups == Cin and Cout = m * Cin: the `depthwise` layer of DepthwiseSeparableConv1D / 2D
# (dual_quaternion_layers.py:19-47).  Descriptor: seld_conv_desc with algebra 1 and groups = Cin.
def make_dwconv_desc(x_shape, cout, kernel, stride, padding, dilation):
    return make_conv_desc(x_shape, cout, 1, kernel, stride, padding, dilation, groups=x_shape[1])


def dwconv_out_shape(desc):
    out = (ctypes.c_int32 * 2)()
    L.check(L.lib().seld_dwconv_out_shape(ctypes.byref(desc), out), "seld_dwconv_out_shape")
    return out[0], out[1]


def dwconv_label(desc, which):
    return kernel_label(L.lib().seld_dwconv_kernel_label, ctypes.byref(desc), which)


def dwconv_work(desc, which):
    """Algorithmic flops / bytes of one call: 2 flops per (output, tap); the streamed operands once -- forward and input
    gradient x + y + weights, weight gradient x + dy + weights."""
    o = dwconv_out_shape(desc)
    s_in, s_out = desc.in_[0] * desc.in_[1], o[0] * o[1]
    K = desc.k[0] * desc.k[1]
    flops = 2.0 * desc.N * desc.Cout * s_out * K
    by = 4.0 * (desc.N * desc.Cin * s_in + desc.N * desc.Cout * s_out + desc.Cout * K)
    return flops, by


def _timed(desc, which):
    return timed(lambda: dwconv_label(desc, which), lambda: dwconv_work(desc, which))


def _dw_y_shape(desc, o, C):
    return (desc.N, C, o[1]) if desc.ndim == 1 else (desc.N, C, o[0], o[1])


def dwconv_fwd(desc, x, w, bias=None):
    x, w, bias = _req(x, "x"), _req(w, "w"), _req(bias, "bias")
    y = torch.empty(_dw_y_shape(desc, dwconv_out_shape(desc), desc.Cout), device=x.device, dtype=torch.float32)
    with _timed(desc, 0):
        L.check(L.lib().seld_dwconv_fwd(ctypes.byref(desc), L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y),
                                        L.current_stream()), "seld_dwconv_fwd")
    return y


def dwconv_bwd_data(desc, dy, w, x_shape):
    dy, w = _req(dy, "dy"), _req(w, "w")
    dx = torch.empty(x_shape, device=dy.device, dtype=torch.float32)
    with _timed(desc, 1):
        L.check(L.lib().seld_dwconv_bwd_data(ctypes.byref(desc), L.ptr(dy), L.ptr(w), L.ptr(dx), L.current_stream()),
                "seld_dwconv_bwd_data")
    return dx


def dwconv_bwd_weight_acc(desc, x, dy, dw, dbias=None):
    """dw += sum x * dy per (channel, tap), dbias += channel sums of dy: per-tile partials in a workspace, one fixed-order
    fold (no atomics, so the same bits with or without SELD_DETERMINISTIC)."""
    x, dy = _req(x, "x"), _req(dy, "dy")
    lib = L.lib()
    nbytes = int(lib.seld_dwconv_bwd_weight_workspace(ctypes.byref(desc)))
    ws = scratch("dwconv", nbytes, x.device)         # the weight-gradient partials (fully rewritten per call)
    with _timed(desc, 2):
        L.check(lib.seld_dwconv_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(dbias),
                                               L.ptr(ws), ws.numel(), L.current_stream()),
                "seld_dwconv_bwd_weight_acc")


class DepthwiseConvFn(torch.autograd.Function):
    """y = conv(x, w, bias, groups=C) for a weight (m*C, 1, k) / (m*C, 1, kh, kw); replaces the depthwise F.conv1d/2d.
    dx: gather-form transposed kernel; dw, dbias: per-tile partials + fold, straight into the optimiser's gradient slots
    when it owns them (_claim_grad_slots), else into a buffer zeroed by seld_step_begin that autograd adds to .grad."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, dilation):
        x = _req(x, "x")
        if w.dim() != x.dim() or w.shape[1] != 1 or w.shape[0] % x.shape[1]:
            raise L.SeldHipError(f"depthwise convolution: weight {tuple(w.shape)} for an input of shape {tuple(x.shape)}")
        if bias is not None and tuple(bias.shape) != (w.shape[0],):
            raise L.SeldHipError(f"depthwise convolution: bias {tuple(bias.shape)} for {w.shape[0]} output channels")
        desc = make_dwconv_desc(tuple(x.shape), w.shape[0], tuple(w.shape[2:]), stride, padding, dilation)
        y = dwconv_fwd(desc, x, w, bias)
        ctx.desc = desc
        ctx.params = (w, bias)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        w, bias = ctx.params
        dy = _req(dy, "dy")
        desc = ctx.desc
        dx = dwconv_bwd_data(desc, dy, w, tuple(x.shape)) if ctx.needs_input_grad[0] else None
        want_w = ctx.needs_input_grad[1]
        want_b = bias is not None and ctx.needs_input_grad[2]
        if not (want_w or want_b):
            return dx, None, None, None, None, None
        if want_w:
            slot, _ = _claim_grad_slots([w] + ([bias] if want_b else []), adjacent=False)
            if slot is not None:
                dwconv_bwd_weight_acc(desc, x, dy, w.grad, bias.grad if want_b else None)
                return dx, None, None, None, None, None
        sizes = [w.numel()] + ([bias.numel()] if want_b else [])
        flat = torch.empty(sum(sizes), device=dy.device, dtype=torch.float32)
        step_begin(flat)
        parts = torch.split(flat, sizes)
        dwconv_bwd_weight_acc(desc, x, dy, parts[0], parts[1] if want_b else None)
        return (dx, parts[0].view(w.shape) if want_w else None, parts[1] if want_b else None, None, None, None)


def depthwise_conv(x, w, bias, stride, padding, dilation):
    """Depthwise convolution (groups = input channels, Cout = m * Cin) of (N, C, T) or (N, C, H, W) input."""
    return DepthwiseConvFn.apply(x, w, bias, stride, padding, dilation)
