"""Transposed 1-D / 2-D convolution (csrc/hc_conv_transpose.hip): descriptor, the three entry points, autograd function."""
import ctypes

import torch

from .. import _lib as L
from ._core import _pair, _req, kernel_label, timed
from .conv import _y_shape, make_conv_desc
from .conv3d import ConvTranspose3dFn
from .norm_act import _direct_targets


# ---- transposed convolution (csrc/hc_conv_transpose.hip) ----------------------------------------------------------------
def conv_transpose_desc(x_shape, cout, algebra, kernel, stride, padding, output_padding, dilation):
    """Descriptor with transposed meaning (Cin / in = the input x) and the int32[2] output padding."""
    desc = make_conv_desc(x_shape, cout, algebra, kernel, stride, padding, dilation)
    op = _pair(output_padding)
    if desc.ndim == 1:
        op = (0, op[1] if isinstance(output_padding, (tuple, list)) else int(output_padding))
    return desc, (ctypes.c_int32 * 2)(*op)


def conv_transpose_out_shape(desc, out_pad):
    out = (ctypes.c_int32 * 2)()
    L.check(L.lib().seld_hc_conv_transpose_out_shape(ctypes.byref(desc), out_pad, out), "seld_hc_conv_transpose_out_shape")
    return out[0], out[1]


def conv_transpose_label(desc, out_pad, which):
    return kernel_label(L.lib().seld_hc_conv_transpose_kernel_label, ctypes.byref(desc), out_pad, which)


def conv_transpose_work(desc, out_pad):
    """Algorithmic flops / bytes of one transposed-convolution call in conv_work's currency: 2*N*Hin*Win*Cin*Cout*kh*kw
    (all 16 Hamilton blocks), x and y once, component weights once."""
    o = conv_transpose_out_shape(desc, out_pad)
    A = desc.algebra
    s_in = desc.in_[0] * desc.in_[1]
    K = desc.k[0] * desc.k[1]
    flops = 2.0 * desc.N * s_in * desc.Cin * desc.Cout * K
    by = 4.0 * (desc.N * desc.Cin * s_in + desc.N * desc.Cout * o[0] * o[1] + desc.Cin * desc.Cout * K // A)
    return flops, by


def _timed(desc, out_pad, which):
    return timed(lambda: conv_transpose_label(desc, out_pad, which), lambda: conv_transpose_work(desc, out_pad))


def conv_transpose_fwd(desc, out_pad, x, ws, bias=None):
    x = _req(x, "x")
    ws = [_req(w, "w") for w in ws]
    bias = _req(bias, "bias")
    o = conv_transpose_out_shape(desc, out_pad)
    y = torch.empty(_y_shape(desc, o), device=x.device, dtype=torch.float32)
    with _timed(desc, out_pad, 0):
        L.check(L.lib().seld_hc_conv_transpose_fwd(ctypes.byref(desc), out_pad, L.ptr(x), L.ptr_array8(ws), L.ptr(bias),
                                                   L.ptr(y), L.current_stream()), "seld_hc_conv_transpose_fwd")
    return y


def conv_transpose_bwd_data(desc, out_pad, dy, ws, x_shape):
    dy = _req(dy, "dy")
    ws = [_req(w, "w") for w in ws]
    dx = torch.empty(x_shape, device=dy.device, dtype=torch.float32)
    with _timed(desc, out_pad, 1):
        L.check(L.lib().seld_hc_conv_transpose_bwd_data(ctypes.byref(desc), out_pad, L.ptr(dy), L.ptr_array8(ws), L.ptr(dx),
                                                        L.current_stream()), "seld_hc_conv_transpose_bwd_data")
    return dx


def conv_transpose_bwd_weight_acc(desc, out_pad, x, dy, dws, dbias=None):
    """dws[c] += weight gradient, dbias += sum of dy.  SELD_DETERMINISTIC=1: the library takes the reproducible path of
    seld_hc_conv_bwd_weight_det (conv_bwd_weight's deterministic branch) with the workspace it asks for."""
    x = _req(x, "x")
    dy = _req(dy, "dy")
    lib = L.lib()
    nbytes = int(lib.seld_hc_conv_transpose_bwd_weight_workspace(ctypes.byref(desc), out_pad))
    wsb = torch.empty(nbytes, device=x.device, dtype=torch.uint8) if nbytes else None
    with _timed(desc, out_pad, 2):
        L.check(lib.seld_hc_conv_transpose_bwd_weight_acc(ctypes.byref(desc), out_pad, L.ptr(x), L.ptr(dy),
                                                          L.ptr_array8(dws), L.ptr(dbias), L.ptr(wsb), nbytes,
                                                          L.current_stream()),
                "seld_hc_conv_transpose_bwd_weight_acc")


class ConvTransposeFn(torch.autograd.Function):
    """y = conv_transpose(x, M, bias) for algebra 1/4; replaces quaternion_transpose_conv / F.conv_transposeNd.
    Backward: dx by the forward convolution, dW by the mirrored convolution's weight gradient, dbias = sum of dy --
    straight into pre-attached gradient slots when the optimiser owns them (_direct_targets), as HyperConvFn."""

    @staticmethod
    def forward(ctx, x, bias, stride, padding, output_padding, dilation, *ws):
        algebra = len(ws)
        k = tuple(ws[0].shape[2:])
        desc, out_pad = conv_transpose_desc(tuple(x.shape), ws[0].shape[1] * algebra, algebra, k, stride, padding,
                                            output_padding, dilation)
        x = _req(x, "x")
        y = conv_transpose_fwd(desc, out_pad, x, ws, bias)
        ctx.desc, ctx.out_pad = desc, out_pad
        ctx.has_bias = bias is not None
        ctx.w_params, ctx.bias_param = ws, bias
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x = ctx.saved_tensors[0]
        ws = ctx.w_params
        dy = _req(dy, "dy")
        desc, out_pad = ctx.desc, ctx.out_pad
        first_w = 6
        dx = conv_transpose_bwd_data(desc, out_pad, dy, ws, tuple(x.shape)) if ctx.needs_input_grad[0] else None
        dws, dbias = [None] * len(ws), None
        want_b = ctx.has_bias and ctx.needs_input_grad[1]
        if any(ctx.needs_input_grad[first_w:]) or want_b:
            direct = _direct_targets(ws, ctx.bias_param)
            if direct is not None:
                conv_transpose_bwd_weight_acc(desc, out_pad, x, dy, direct[0], direct[1])
            else:
                dws = [torch.zeros_like(w) for w in ws]
                dbias = torch.zeros_like(ctx.bias_param) if want_b else None
                conv_transpose_bwd_weight_acc(desc, out_pad, x, dy, dws, dbias)
                dws = [g if need else None for g, need in zip(dws, ctx.needs_input_grad[first_w:])]
        return (dx, dbias, None, None, None, None, *dws)


def hyper_conv_transpose(x, ws, bias, stride, padding, output_padding, dilation):
    """Transposed convolution y = conv_transpose(x, M(ws), bias, stride, padding, output_padding, dilation) on the HIP
    kernels; ws: 1 (real) or 4 (quaternion) component tensors (Cin/A, Cout/A, *k)."""
    if len(ws) not in (1, 4):
        raise L.SeldHipError("transposed convolution: algebra 1 or 4 (the reference has no dual-quaternion form)")
    if x.dim() == 5:
        return ConvTranspose3dFn.apply(x, bias, stride, padding, output_padding, dilation, *ws)
    return ConvTransposeFn.apply(x, bias, stride, padding, output_padding, dilation, *ws)
