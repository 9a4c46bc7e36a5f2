"""3-D convolution and transposed convolution (csrc/hc_conv3d.hip): descriptor, the three entry points, autograd functions."""
import ctypes

import torch

from .. import _lib as L
from ._core import _req, kernel_label, timed
from .norm_act import _direct_targets
from .train_ops import step_begin


# ---- 3-D convolution and transposed convolution (csrc/hc_conv3d.hip) -----------------------------------------------------
# One descriptor type for both; out_pad None selects the convolution's entry points, an int32[3] the transposed ones.
def _triple(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 3:
            raise L.SeldHipError(f"convolution3d: {what} needs 3 values, got {tuple(v)}")
        return tuple(int(a) for a in v)
    return (int(v),) * 3


def make_conv3d_desc(x_shape, cout, algebra, kernel, stride, padding, dilation, groups=1):
    """x_shape: (N, C, D, H, W).  kernel/stride/padding/dilation: int or 3-tuple."""
    if len(x_shape) != 5:
        raise L.SeldHipError(f"convolution3d: expected a 5-D input, got shape {tuple(x_shape)}")
    d = L.Conv3dDesc()
    d.algebra, d.N, d.Cin, d.Cout, d.groups = algebra, x_shape[0], x_shape[1], cout, groups
    k, s, p, dl = (_triple(kernel, "kernel_size"), _triple(stride, "stride"), _triple(padding, "padding"),
                   _triple(dilation, "dilatation"))
    for i in range(3):
        d.in_[i], d.k[i], d.stride[i], d.pad[i], d.dil[i] = x_shape[2 + i], k[i], s[i], p[i], dl[i]
    return d


def conv3d_transpose_desc(x_shape, cout, algebra, kernel, stride, padding, output_padding, dilation):
    """Descriptor with transposed meaning (Cin / in = the input x) and the int32[3] output padding."""
    desc = make_conv3d_desc(x_shape, cout, algebra, kernel, stride, padding, dilation)
    return desc, (ctypes.c_int32 * 3)(*_triple(output_padding, "output_padding"))


def conv3d_out_shape(desc, out_pad=None):
    out = (ctypes.c_int32 * 3)()
    lib = L.lib()
    if out_pad is None:
        L.check(lib.seld_hc_conv3d_out_shape(ctypes.byref(desc), out), "seld_hc_conv3d_out_shape")
    else:
        L.check(lib.seld_hc_conv3d_transpose_out_shape(ctypes.byref(desc), out_pad, out),
                "seld_hc_conv3d_transpose_out_shape")
    return out[0], out[1], out[2]


def conv3d_label(desc, out_pad, which):
    if out_pad is None:
        return kernel_label(L.lib().seld_hc_conv3d_kernel_label, ctypes.byref(desc), which)
    return kernel_label(L.lib().seld_hc_conv3d_transpose_kernel_label, ctypes.byref(desc), out_pad, which)


def conv3d_work(desc, out_pad=None):
    """Algorithmic flops / bytes of one 3-D call: 2*N*Cout*Cin*kd*kh*kw per position of the convolution's output (the
    transposed convolution's input), all Hamilton blocks; x and y once, component weights once."""
    o = conv3d_out_shape(desc, out_pad)
    s_in = desc.in_[0] * desc.in_[1] * desc.in_[2]
    s_out = o[0] * o[1] * o[2]
    K = desc.k[0] * desc.k[1] * desc.k[2]
    flops = 2.0 * desc.N * desc.Cin * desc.Cout * K * (s_out if out_pad is None else s_in)
    by = 4.0 * (desc.N * desc.Cin * s_in + desc.N * desc.Cout * s_out + desc.Cin * desc.Cout * K // desc.algebra)
    return flops, by


def _timed(desc, out_pad, which):
    return timed(lambda: conv3d_label(desc, out_pad, which), lambda: conv3d_work(desc, out_pad))


def conv3d_fwd(desc, out_pad, x, ws, bias=None):
    x = _req(x, "x")
    ws = [_req(w, "w") for w in ws]
    bias = _req(bias, "bias")
    y = torch.empty((desc.N, desc.Cout) + conv3d_out_shape(desc, out_pad), device=x.device, dtype=torch.float32)
    lib = L.lib()
    with _timed(desc, out_pad, 0):
        if out_pad is None:
            L.check(lib.seld_hc_conv3d_fwd(ctypes.byref(desc), L.ptr(x), L.ptr_array8(ws), L.ptr(bias), L.ptr(y),
                                           L.current_stream()), "seld_hc_conv3d_fwd")
        else:
            L.check(lib.seld_hc_conv3d_transpose_fwd(ctypes.byref(desc), out_pad, L.ptr(x), L.ptr_array8(ws), L.ptr(bias),
                                                     L.ptr(y), L.current_stream()), "seld_hc_conv3d_transpose_fwd")
    return y


def conv3d_bwd_data(desc, out_pad, dy, ws, x_shape):
    dy = _req(dy, "dy")
    ws = [_req(w, "w") for w in ws]
    dx = torch.empty(x_shape, device=dy.device, dtype=torch.float32)
    lib = L.lib()
    with _timed(desc, out_pad, 1):
        if out_pad is None:
            L.check(lib.seld_hc_conv3d_bwd_data(ctypes.byref(desc), L.ptr(dy), L.ptr_array8(ws), L.ptr(dx),
                                                L.current_stream()), "seld_hc_conv3d_bwd_data")
        else:
            L.check(lib.seld_hc_conv3d_transpose_bwd_data(ctypes.byref(desc), out_pad, L.ptr(dy), L.ptr_array8(ws),
                                                          L.ptr(dx), L.current_stream()),
                    "seld_hc_conv3d_transpose_bwd_data")
    return dx


def conv3d_bwd_weight_acc(desc, out_pad, x, dy, dws, dbias=None):
    """dws[c] += weight gradient, dbias += channel sums of dy: position-split partials in a workspace, one fixed-order
    fold (no atomics, so the same bits with or without SELD_DETERMINISTIC)."""
    x = _req(x, "x")
    dy = _req(dy, "dy")
    lib = L.lib()
    if out_pad is None:
        nbytes = int(lib.seld_hc_conv3d_bwd_weight_workspace(ctypes.byref(desc)))
    else:
        nbytes = int(lib.seld_hc_conv3d_transpose_bwd_weight_workspace(ctypes.byref(desc), out_pad))
    wsb = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    with _timed(desc, out_pad, 2):
        if out_pad is None:
            L.check(lib.seld_hc_conv3d_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(dy), L.ptr_array8(dws),
                                                      L.ptr(dbias), L.ptr(wsb), nbytes,
                                                      L.current_stream()), "seld_hc_conv3d_bwd_weight_acc")
        else:
            L.check(lib.seld_hc_conv3d_transpose_bwd_weight_acc(ctypes.byref(desc), out_pad, L.ptr(x), L.ptr(dy),
                                                                L.ptr_array8(dws), L.ptr(dbias), L.ptr(wsb), nbytes,
                                                                L.current_stream()),
                    "seld_hc_conv3d_transpose_bwd_weight_acc")


def _conv3d_weights(ws, x, transposed):
    """The component tensors must agree with each other and with the input's channels: the kernels index them by the
    descriptor alone."""
    A = len(ws)
    shape = tuple(ws[0].shape)
    if len(shape) != 5 or any(tuple(w.shape) != shape for w in ws):
        raise L.SeldHipError(f"convolution3d: component tensors {[tuple(w.shape) for w in ws]}, expected {A} equal 5-D")
    if shape[0 if transposed else 1] * A != x.shape[1]:
        raise L.SeldHipError(f"convolution3d: input of {x.shape[1]} channels, component tensors {shape} (algebra {A})")


def _conv3d_backward(ctx, dy, first_w):
    """dx, dbias, dws of HyperConv3dFn / ConvTranspose3dFn.  The weight gradient goes into the optimiser's gradient slots
    when it owns them (_direct_targets), else into fresh buffers zeroed by seld_step_begin: no ATen launch either way."""
    x = ctx.saved_tensors[0]
    ws = ctx.w_params
    dy = _req(dy, "dy")
    desc, out_pad = ctx.desc, ctx.out_pad
    dx = conv3d_bwd_data(desc, out_pad, dy, ws, tuple(x.shape)) if ctx.needs_input_grad[0] else None
    dws, dbias = [None] * len(ws), None
    want_b = ctx.has_bias and ctx.needs_input_grad[1]
    if any(ctx.needs_input_grad[first_w:]) or want_b:
        direct = _direct_targets(ws, ctx.bias_param)
        if direct is not None:
            conv3d_bwd_weight_acc(desc, out_pad, x, dy, direct[0], direct[1])
        else:
            sizes = [w.numel() for w in ws] + ([ctx.bias_param.numel()] if want_b else [])
            flat = torch.empty(sum(sizes), device=dy.device, dtype=torch.float32)
            step_begin(flat)
            parts = list(torch.split(flat, sizes))
            dws = [p.view(w.shape) for p, w in zip(parts, ws)]
            dbias = parts[-1] if want_b else None
            conv3d_bwd_weight_acc(desc, out_pad, x, dy, dws, dbias)
            dws = [g if need else None for g, need in zip(dws, ctx.needs_input_grad[first_w:])]
    return dx, dbias, dws


class HyperConv3dFn(torch.autograd.Function):
    """y = W (x) x on 5-D input for algebra 1/4/8; replaces the F.conv3d of quaternion_conv / dual_quaternion_conv.
    Forward: implicit-GEMM kernel; dx: stride-phase kernel; dW, dbias: partials + fold (csrc/hc_conv3d.hip)."""

    @staticmethod
    def forward(ctx, x, bias, stride, padding, dilation, *ws):
        x = _req(x, "x")
        _conv3d_weights(ws, x, False)
        algebra = len(ws)
        desc = make_conv3d_desc(tuple(x.shape), ws[0].shape[0] * algebra, algebra, tuple(ws[0].shape[2:]), stride,
                                padding, dilation)
        y = conv3d_fwd(desc, None, x, ws, bias)
        ctx.desc, ctx.out_pad = desc, None
        ctx.has_bias = bias is not None
        ctx.w_params, ctx.bias_param = ws, bias
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dbias, dws = _conv3d_backward(ctx, dy, 5)
        return (dx, dbias, None, None, None, *dws)


class ConvTranspose3dFn(torch.autograd.Function):
    """y = conv_transpose(x, M, bias) on 5-D input for algebra 1/4; replaces the F.conv_transpose3d of
    quaternion_transpose_conv.  Forward: stride-phase kernel; dx: implicit-GEMM kernel; dW: the mirrored convolution's
    partials + fold, dbias = channel sums of dy."""

    @staticmethod
    def forward(ctx, x, bias, stride, padding, output_padding, dilation, *ws):
        x = _req(x, "x")
        _conv3d_weights(ws, x, True)
        algebra = len(ws)
        desc, out_pad = conv3d_transpose_desc(tuple(x.shape), ws[0].shape[1] * algebra, algebra, tuple(ws[0].shape[2:]),
                                              stride, padding, output_padding, dilation)
        y = conv3d_fwd(desc, out_pad, x, ws, bias)
        ctx.desc, ctx.out_pad = desc, out_pad
        ctx.has_bias = bias is not None
        ctx.w_params, ctx.bias_param = ws, bias
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dbias, dws = _conv3d_backward(ctx, dy, 6)
        return (dx, dbias, None, None, None, None, *dws)
