"""Element-wise quaternion algebra (csrc/quat_algebra.hip) and the quaternion rotation weight (csrc/quat_rotation.hip)."""
import ctypes

import torch

from .. import _lib as L
from ._core import _req, scratch
from .conv import hyper_conv
from .conv_transpose import hyper_conv_transpose
from .linear_mha import hyper_linear
from .norm_act import _claim_grad_slots


# ---- element-wise quaternion algebra (csrc/quat_algebra.hip) --------------------------------------------------------
# get_modulus / get_normalized / hamilton_product / q_normalize / quaternion_exp of the two *_ops modules: one kernel per
# op and direction over the input seen as (dim0, mid, 4, M) (seld_quat_shape), whatever its rank.
def quat_shape(x):
    """seld_quat_shape of a rank 2..5 tensor: the component axis is the last one below rank 4, else axis 1."""
    if x.dim() not in (2, 3, 4, 5):
        raise L.SeldHipError(f"quaternion algebra: expected an input of 2 to 5 dimensions, got {x.dim()}")
    s = tuple(int(v) for v in x.shape)
    if x.dim() == 2:
        dims = (s[0], 1, s[1], 1)
    elif x.dim() == 3:
        dims = (s[0], s[1], s[2], 1)
    else:
        inner = 1
        for v in s[2:]:
            inner *= v
        dims = (s[0], 1, s[1], inner)
    if min(dims) < 1 or max(dims) >= 2 ** 31:
        raise L.SeldHipError(f"quaternion algebra: unsupported shape {s}")
    return L.QuatShape(*dims)


def _quat_summed_shape(x):
    """Shape of a result summed over dim 0: the input's without dim 0 and with the component axis divided by 4."""
    s = list(x.shape)
    s[-1 if x.dim() < 4 else 1] //= 4
    return tuple(s[1:])


def _quat_cat1_shape(x):
    """Shape of q_normalize / quaternion_exp's result: the components concatenated on dim 1."""
    if x.dim() == 3:
        return (x.shape[0], 4 * x.shape[1], x.shape[2] // 4)
    return tuple(x.shape)


def _quat_ws(qs, device):
    """Workspace of the dim-0 partials (fully rewritten per call)."""
    nbytes = int(L.lib().seld_quat_reduce_workspace(ctypes.byref(qs)))
    if nbytes == 0:
        raise L.SeldHipError("seld_quat_reduce_workspace: refused shape "
                             f"{(qs.dim0, qs.mid, qs.comp, qs.inner)} (component axis not divisible by 4, or too large)")
    return scratch("quat", nbytes, device)


def _quat_modulus_sum(qs, x):
    y = torch.empty(_quat_summed_shape(x), device=x.device, dtype=torch.float32)
    ws = _quat_ws(qs, x.device)
    L.check(L.lib().seld_quat_modulus_sum_fwd(ctypes.byref(qs), L.ptr(x), L.ptr(y), L.ptr(ws), ws.numel(),
                                              L.current_stream()),
            "seld_quat_modulus_sum_fwd")
    return y


class QuatModulusFn(torch.autograd.Function):
    """|q| per quaternion (vector_form) or the root of its square summed over dim 0 (the reference's default)."""

    @staticmethod
    def forward(ctx, x, vector_form):
        x = _req(x, "input")
        qs = quat_shape(x)
        if vector_form:
            y = torch.empty((x.shape[0],) + _quat_summed_shape(x), device=x.device, dtype=torch.float32)
            L.check(L.lib().seld_quat_modulus_fwd(ctypes.byref(qs), L.ptr(x), L.ptr(y), L.current_stream()),
                    "seld_quat_modulus_fwd")
            ctx.save_for_backward(x)
        else:
            y = _quat_modulus_sum(qs, x)
            ctx.save_for_backward(x, y)
        ctx.qs, ctx.vector_form = qs, vector_form
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        x = ctx.saved_tensors[0]
        dx = torch.empty_like(x)
        if ctx.vector_form:
            L.check(L.lib().seld_quat_modulus_bwd(ctypes.byref(ctx.qs), L.ptr(x), L.ptr(dy), L.ptr(dx),
                                                  L.current_stream()), "seld_quat_modulus_bwd")
        else:
            L.check(L.lib().seld_quat_modulus_sum_bwd(ctypes.byref(ctx.qs), L.ptr(x), L.ptr(ctx.saved_tensors[1]),
                                                      L.ptr(dy), L.ptr(dx), L.current_stream()),
                    "seld_quat_modulus_sum_bwd")
        return dx, None


def quat_modulus(x, vector_form=False):
    return QuatModulusFn.apply(x, bool(vector_form))


class QuatNormalizedFn(torch.autograd.Function):
    """x / (modulus summed over dim 0, broadcast over dim 0 and the components, + eps)."""

    @staticmethod
    def forward(ctx, x, eps):
        x = _req(x, "input")
        qs = quat_shape(x)
        mod = _quat_modulus_sum(qs, x)
        y = torch.empty_like(x)
        L.check(L.lib().seld_quat_normalized_fwd(ctypes.byref(qs), L.ptr(x), L.ptr(mod), eps, L.ptr(y),
                                                 L.current_stream()), "seld_quat_normalized_fwd")
        ctx.save_for_backward(x, mod)
        ctx.qs, ctx.eps = qs, eps
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        x, mod = ctx.saved_tensors
        dx = torch.empty_like(x)
        ws = _quat_ws(ctx.qs, x.device)
        L.check(L.lib().seld_quat_normalized_bwd(ctypes.byref(ctx.qs), L.ptr(x), L.ptr(mod), L.ptr(dy), ctx.eps,
                                                 L.ptr(dx), L.ptr(ws), ws.numel(), L.current_stream()),
                "seld_quat_normalized_bwd")
        return dx, None


def quat_normalized(x, eps=0.0001):
    return QuatNormalizedFn.apply(x, float(eps))


class _QuatUnaryFn(torch.autograd.Function):
    """q_normalize / quaternion_exp: the result has the components concatenated on dim 1 (cat1) or the input's layout."""

    @staticmethod
    def forward(ctx, x, op, cat1):
        x = _req(x, "input")
        qs = quat_shape(x)
        layout = L.SELD_QUAT_LAYOUT_CAT1 if cat1 else L.SELD_QUAT_LAYOUT_INPUT
        y = torch.empty(_quat_cat1_shape(x) if cat1 else tuple(x.shape), device=x.device, dtype=torch.float32)
        L.check(getattr(L.lib(), f"seld_quat_{op}_fwd")(ctypes.byref(qs), layout, L.ptr(x), L.ptr(y), L.current_stream()),
                f"seld_quat_{op}_fwd")
        ctx.save_for_backward(x)
        ctx.qs, ctx.op, ctx.layout = qs, op, layout
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        x, = ctx.saved_tensors
        dx = torch.empty_like(x)
        L.check(getattr(L.lib(), f"seld_quat_{ctx.op}_bwd")(ctypes.byref(ctx.qs), ctx.layout, L.ptr(x), L.ptr(dy),
                                                            L.ptr(dx), L.current_stream()), f"seld_quat_{ctx.op}_bwd")
        return dx, None, None


def quat_unit(x, cat1=True):
    """x_c / sqrt(|q|^2 + 1e-4)."""
    return _QuatUnaryFn.apply(x, "normalize", bool(cat1))


def quat_exp(x, cat1=True):
    """exp(r) * [cos n, (i, j, k) sin(n) / n], n = |(i, j, k)| + 1e-4."""
    return _QuatUnaryFn.apply(x, "exp", bool(cat1))


class HamiltonProductFn(torch.autograd.Function):
    """q0 (x) q1 of two tensors of one shape; backward: both gradients from one kernel."""

    @staticmethod
    def forward(ctx, q0, q1):
        q0, q1 = _req(q0, "q0"), _req(q1, "q1")
        if q0.shape != q1.shape:
            raise L.SeldHipError(f"hamilton_product: shapes differ: {tuple(q0.shape)} and {tuple(q1.shape)}")
        qs = quat_shape(q0)
        y = torch.empty_like(q0)
        L.check(L.lib().seld_quat_hamilton_fwd(ctypes.byref(qs), L.ptr(q0), L.ptr(q1), L.ptr(y), L.current_stream()),
                "seld_quat_hamilton_fwd")
        ctx.save_for_backward(q0, q1)
        ctx.qs = qs
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        q0, q1 = ctx.saved_tensors
        d0, d1 = torch.empty_like(q0), torch.empty_like(q1)
        L.check(L.lib().seld_quat_hamilton_bwd(ctypes.byref(ctx.qs), L.ptr(q0), L.ptr(q1), L.ptr(dy), L.ptr(d0), L.ptr(d1),
                                               L.current_stream()), "seld_quat_hamilton_bwd")
        return d0, d1


def hamilton_product(q0, q1):
    if q0.shape != q1.shape:
        q0, q1 = torch.broadcast_tensors(q0, q1)
    return HamiltonProductFn.apply(q0, q1)


# ---- quaternion rotation weight (csrc/quat_rotation.hip) -----------------------------------------------------------------
# quaternion_{conv,transpose_conv,linear}_rotation (quaternion_ops.py:174-388) build ONE real weight K from the four
# component tensors and run one real op with it: here K comes from seld_quat_rotation_form and the op is the algebra-1
# convolution / transposed convolution / SELD_LIN_REAL linear above, with their own backward, deterministic mode and
# capture.  RotationWeightFn folds dK back onto the components.
def _rot_dims(ws, layout):
    """(A, B, taps, shape) of the component tensors (A, B, *taps); 2-D for the linear layout."""
    if len(ws) != 4 or any(w is None for w in ws):
        raise L.SeldHipError("rotation: needs the four component tensors r, i, j, k")
    shape = tuple(ws[0].shape)
    if any(tuple(w.shape) != shape for w in ws):
        raise L.SeldHipError(f"rotation: component shapes differ: {[tuple(w.shape) for w in ws]}")
    if len(shape) < 2 or (layout == L.SELD_ROT_LAYOUT_LINEAR and len(shape) != 2):
        raise L.SeldHipError(f"rotation: bad component shape {shape}")
    taps = 1
    for s in shape[2:]:
        taps *= int(s)
    return int(shape[0]), int(shape[1]), taps, shape


def rotation_weight_shape(layout, qformat, w_shape):
    """K (MB*A, MB*B, *taps) for SELD_ROT_LAYOUT_CONV, K^T (MB*B, MB*A) for SELD_ROT_LAYOUT_LINEAR; MB = 4 with
    quaternion_format, else 3."""
    m = 4 if qformat else 3
    if layout == L.SELD_ROT_LAYOUT_CONV:
        return (m * w_shape[0], m * w_shape[1]) + tuple(w_shape[2:])
    return (m * w_shape[1], m * w_shape[0])


def rotation_form(layout, qformat, ws):
    A, B, taps, shape = _rot_dims(ws, layout)
    ws = [_req(w, "w") for w in ws]
    K = torch.empty(rotation_weight_shape(layout, qformat, shape), device=ws[0].device, dtype=torch.float32)
    L.check(L.lib().seld_quat_rotation_form(layout, int(bool(qformat)), A, B, taps, L.ptr_array8(ws), L.ptr(K),
                                            L.current_stream()), "seld_quat_rotation_form")
    return K


def rotation_form_bwd(layout, qformat, ws, dK, dws, accumulate):
    """dws[c] = (accumulate: +=) dL/dw_c from dK."""
    A, B, taps, _ = _rot_dims(ws, layout)
    ws = [_req(w, "w") for w in ws]
    dK = _req(dK, "dK")
    L.check(L.lib().seld_quat_rotation_form_bwd(layout, int(bool(qformat)), A, B, taps, L.ptr_array8(ws), L.ptr(dK),
                                                L.ptr_array8(dws), int(bool(accumulate)), L.current_stream()),
            "seld_quat_rotation_form_bwd")


class RotationWeightFn(torch.autograd.Function):
    """K = rotation weight of (r, i, j, k).  Backward: one kernel, each element's four gradients from its own entries of
    dK (no atomics), straight into the optimiser's gradient slots when it owns all four (_claim_grad_slots), else into
    fresh tensors for autograd."""

    @staticmethod
    def forward(ctx, layout, qformat, *ws):
        wc = [_req(w, "w") for w in ws]
        ctx.layout, ctx.qformat, ctx.params = layout, qformat, ws
        ctx.save_for_backward(*wc)
        return rotation_form(layout, qformat, wc)

    @staticmethod
    def backward(ctx, dK):
        ws = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        params = ctx.params
        if all(need) and all(p.is_contiguous() for p in params):
            slot, clean = _claim_grad_slots(params, adjacent=False)
            if slot is not None and all(p.grad.is_contiguous() for p in params):
                rotation_form_bwd(ctx.layout, ctx.qformat, ws, dK, [p.grad for p in params], accumulate=not clean)
                return (None, None) + (None,) * len(ws)
        dws = [torch.empty_like(w) for w in ws]
        rotation_form_bwd(ctx.layout, ctx.qformat, ws, dK, dws, accumulate=False)
        return (None, None) + tuple(g if n else None for g, n in zip(dws, need))


def _rot_check(what, channels, want_channels, bias, out_channels, m):
    if channels != want_channels:
        raise L.SeldHipError(f"{what}: the input has {channels} channels, the rotation weight takes {want_channels} "
                             f"({m} x the component tensors' {want_channels // m}; quaternion_format gives 4, else 3)")
    if bias is not None and (bias.dim() != 1 or bias.numel() != out_channels):
        raise L.SeldHipError(f"{what}: bias of shape {tuple(bias.shape)}, the op has {out_channels} output channels "
                             f"(the reference's F.conv / addmm call needs as many)")


def hyper_conv_rotation(x, ws, bias, stride, padding, dilation, qformat):
    """quaternion_conv_rotation: F.convNd(x, K, bias), K (MB*O, MB*I, *k) the rotation weight of (O, I, *k) components."""
    A, B, _, shape = _rot_dims(ws, L.SELD_ROT_LAYOUT_CONV)
    m = 4 if qformat else 3
    if len(shape) != x.dim():
        raise L.SeldHipError(f"quaternion_conv_rotation: {x.dim()}-D input, {len(shape)}-D component weights")
    _rot_check("quaternion_conv_rotation", int(x.shape[1]), m * B, bias, m * A, m)
    K = RotationWeightFn.apply(L.SELD_ROT_LAYOUT_CONV, bool(qformat), *ws)
    return hyper_conv(x, (K,), bias, stride, padding, dilation)


def hyper_conv_transpose_rotation(x, ws, bias, stride, padding, output_padding, dilation, qformat):
    """quaternion_transpose_conv_rotation: F.conv_transposeNd(x, K, bias), K (MB*Iin, MB*Oout, *k) the rotation weight of
    (Iin, Oout, *k) components."""
    A, B, _, shape = _rot_dims(ws, L.SELD_ROT_LAYOUT_CONV)
    m = 4 if qformat else 3
    if len(shape) != x.dim():
        raise L.SeldHipError(f"quaternion_transpose_conv_rotation: {x.dim()}-D input, {len(shape)}-D component weights")
    _rot_check("quaternion_transpose_conv_rotation", int(x.shape[1]), m * A, bias, m * B, m)
    K = RotationWeightFn.apply(L.SELD_ROT_LAYOUT_CONV, bool(qformat), *ws)
    return hyper_conv_transpose(x, (K,), bias, stride, padding, output_padding, dilation)


def hyper_linear_rotation(x, ws, bias, qformat):
    """quaternion_linear_rotation: x @ K + bias, K (MB*I, MB*O) the rotation weight of (I, O) components; the real linear
    kernel takes K^T, which the form kernel writes directly."""
    A, B, _, _ = _rot_dims(ws, L.SELD_ROT_LAYOUT_LINEAR)
    m = 4 if qformat else 3
    _rot_check("quaternion_linear_rotation", int(x.shape[-1]) if x.dim() else 0, m * A, bias, m * B, m)
    W = RotationWeightFn.apply(L.SELD_ROT_LAYOUT_LINEAR, bool(qformat), *ws)
    return hyper_linear(x, (W,), bias, L.SELD_LIN_REAL)
