"""Hypercomplex linear layers and the attention core (csrc/hc_linear.hip, csrc/mha*.hip)."""
import ctypes

import torch

from .. import _lib as L
from ._core import _req
from .norm_act import _claim_grad_slots


# ======================================================================================
# linear layers
# ======================================================================================
class HyperLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, kind, *ws):
        x2 = _req(x.reshape(-1, x.shape[-1]), "x")
        rows, in_f = x2.shape
        if kind == L.SELD_LIN_REAL:
            out_f = ws[0].shape[0]
        else:
            out_f = ws[0].shape[1] * kind
        ctx.params = (bias, tuple(ws))
        ws = [_req(w, "w") for w in ws]
        y = torch.empty((rows, out_f), device=x.device, dtype=torch.float32)
        L.check(L.lib().seld_hc_linear_fwd(kind, rows, in_f, out_f, L.ptr(x2), L.ptr_array8(ws), L.ptr(_req(bias, "bias")),
                                           L.ptr(y), L.current_stream()), "seld_hc_linear_fwd")
        ctx.meta = (kind, rows, in_f, out_f, tuple(x.shape), bias is not None)
        ctx.save_for_backward(x2, *ws)
        return y.reshape(*x.shape[:-1], out_f)

    @staticmethod
    def backward(ctx, dy):
        kind, rows, in_f, out_f, xshape, has_bias = ctx.meta
        x2, *ws = ctx.saved_tensors
        bias_p, ws_p = ctx.params
        dy2 = _req(dy.reshape(rows, out_f), "dy")
        dev = dy2.device
        dx = torch.empty((rows, in_f), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        need_w = any(ctx.needs_input_grad[3:])
        need_b = has_bias and ctx.needs_input_grad[1]
        # The kernel WRITES the parameter gradients: it may write them straight into flat-gradient slots that are
        # still zero (first and only use of the layer since zero_grad); otherwise autograd accumulates.
        direct = False
        if need_w and (need_b or not has_bias) and all(w.is_contiguous() for w in ws_p):
            slot, clean = _claim_grad_slots(list(ws_p) + ([bias_p] if has_bias else []), adjacent=False)
            direct = slot is not None and clean
        if direct:
            dws, dbias = [w.grad for w in ws_p], (bias_p.grad if has_bias else None)
        else:
            dws = [torch.empty_like(w) for w in ws] if need_w else None
            dbias = torch.empty(out_f, device=dev, dtype=torch.float32) if need_b else None
        nbytes = L.lib().seld_hc_linear_bwd_workspace(kind, in_f, out_f)
        wsb = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
        L.check(L.lib().seld_hc_linear_bwd(kind, rows, in_f, out_f, L.ptr(x2), L.ptr(dy2), L.ptr_array8(ws), L.ptr(dx),
                                           L.ptr_array8(dws) if dws is not None else None, L.ptr(dbias), L.ptr(wsb),
                                           nbytes, L.current_stream()), "seld_hc_linear_bwd")
        dxr = dx.reshape(xshape) if dx is not None else None
        if direct:
            return (dxr, None, None, *([None] * len(ws)))
        return (dxr, dbias, None, *(dws if dws is not None else [None] * len(ws)))


def hyper_linear(x, ws, bias, kind):
    return HyperLinearFn.apply(x, bias, kind, *ws)


# ======================================================================================
# attention core
# ======================================================================================
class MhaCoreFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(hd)) v on (N, E, T) tensors (model.py:39-48)."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        q, k, v = _req(q, "q"), _req(k, "k"), _req(v, "v")
        N, E, T = q.shape
        hd = E // heads
        out = torch.empty_like(q)
        lse = torch.empty((N, heads, T), device=q.device, dtype=torch.float32)
        L.check(L.lib().seld_mha_fwd(L.ptr(q), L.ptr(k), L.ptr(v), N, T, heads, hd, L.ptr(out), L.ptr(lse),
                                     L.current_stream()), "seld_mha_fwd")
        ctx.geom = (N, T, heads, hd)
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        N, T, H, hd = ctx.geom
        dout = _req(dout, "dout")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        lib = L.lib()
        nbytes = lib.seld_mha_bwd_workspace(N, T, H)
        wsb = torch.empty((nbytes + 3) // 4, device=q.device, dtype=torch.float32)
        L.check(lib.seld_mha_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(dout), L.ptr(lse), N, T, H, hd,
                                 L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(wsb), nbytes,
                                 L.current_stream()), "seld_mha_bwd")
        return dq, dk, dv, None


def mha_core(q, k, v, heads):
    return MhaCoreFn.apply(q, k, v, heads)


def _mha_keep_mask(mask, shape, device):
    """The mask of model.py:43-44 as (uint8 keep tensor, int64[4] element strides) over the energy shape (N, H, Tq, Tk).
    It broadcasts with torch's rules (a 2-D mask is (Tq, Tk); a 3-D mask's first dim lines up with the heads) and must
    not enlarge the energy shape.  bool / uint8 masks are read as they are; any other dtype is converted once with
    `mask != 0`, the only ATen launch on this path.  Shapes only: no host synchronisation."""
    if not torch.is_tensor(mask):
        raise L.SeldHipError(f"attention mask: expected a tensor, got {type(mask).__name__}")
    if mask.device != device:
        raise L.SeldHipError(f"attention mask: on {mask.device}, the attention runs on {device}")
    try:
        ok = mask.dim() <= 4 and tuple(torch.broadcast_shapes(tuple(mask.shape), shape)) == tuple(shape)
    except RuntimeError:
        ok = False
    if not ok:
        raise L.SeldHipError(f"attention mask: shape {tuple(mask.shape)} does not broadcast to the energy {tuple(shape)}")
    if mask.dtype == torch.bool:
        keep = mask.view(torch.uint8)
    elif mask.dtype == torch.uint8:
        keep = mask
    else:
        keep = mask != 0
        keep = keep.view(torch.uint8)
    strides = (ctypes.c_int64 * 4)(*keep.expand(shape).stride())
    return keep, strides


class MhaMaskedFn(torch.autograd.Function):
    """softmax(masked(q k^T) / sqrt(hd)) v (model.py:25-51 with a mask) on q (N, E, Tq) and k, v (N, E, Tk):
    seld_mha_fwd_ex / seld_mha_bwd_ex.  Masked scores take -1e9 / sqrt(hd); the mask has no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, heads, mask):
        q, k, v = _req(q, "q"), _req(k, "k"), _req(v, "v")
        if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
            raise L.SeldHipError("mha_core_ex: expected (N, E, T) tensors")
        N, E, Tq = q.shape
        Tk = k.shape[2]
        if tuple(k.shape) != (N, E, Tk) or tuple(v.shape) != (N, E, v.shape[2]):
            raise L.SeldHipError(f"mha_core_ex: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not match")
        if v.shape[2] != Tk:
            raise L.SeldHipError(f"mha_core_ex: value_len {v.shape[2]} != key_len {Tk}")
        if heads <= 0 or E % heads:
            raise L.SeldHipError(f"mha_core_ex: {E} channels do not split into {heads} heads")
        hd = E // heads
        if hd > 64:
            raise L.SeldHipError(f"mha_core_ex: head dim {hd} > 64 is not supported")
        keep, strides = (None, None) if mask is None else _mha_keep_mask(mask, (N, heads, Tq, Tk), q.device)
        out = torch.empty_like(q)
        lse = torch.empty((N, heads, Tq), device=q.device, dtype=torch.float32)
        L.check(L.lib().seld_mha_fwd_ex(L.ptr(q), L.ptr(k), L.ptr(v), N, Tq, Tk, heads, hd, L.ptr(keep), strides,
                                        L.ptr(out), L.ptr(lse), L.current_stream()), "seld_mha_fwd_ex")
        ctx.geom = (N, Tq, Tk, heads, hd)
        ctx.strides = strides
        ctx.save_for_backward(q, k, v, out, lse, keep)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, keep = ctx.saved_tensors
        N, Tq, Tk, H, hd = ctx.geom
        dout = _req(dout, "dout")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        lib = L.lib()
        nbytes = lib.seld_mha_bwd_ex_workspace(N, Tq, H)
        wsb = torch.empty((nbytes + 3) // 4, device=q.device, dtype=torch.float32)
        L.check(lib.seld_mha_bwd_ex(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(dout), L.ptr(lse), N, Tq, Tk, H, hd,
                                    L.ptr(keep), ctx.strides, L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(wsb), nbytes,
                                    L.current_stream()), "seld_mha_bwd_ex")
        return dq, dk, dv, None, None


def mha_core_ex(q, k, v, heads, mask=None):
    """Attention with an optional mask (broadcast to (N, heads, Tq, Tk), entries == 0 masked) and key_len != query_len."""
    return MhaMaskedFn.apply(q, k, v, heads, mask)


class MhaPackedFn(torch.autograd.Function):
    """The same attention on ONE projected tensor qkv (N, 3E, T) = [values | keys | queries] (seld_mha_fwd_packed): the
    three projections of model.py:31-33 are one convolution, and so are their data and weight gradients."""

    @staticmethod
    def forward(ctx, qkv, heads):
        qkv = _req(qkv, "qkv")
        N, E3, T = qkv.shape
        E = E3 // 3
        hd = E // heads
        out = torch.empty((N, E, T), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((N, heads, T), device=qkv.device, dtype=torch.float32)
        L.check(L.lib().seld_mha_fwd_packed(L.ptr(qkv), N, T, heads, hd, L.ptr(out), L.ptr(lse), L.current_stream()),
                "seld_mha_fwd_packed")
        ctx.geom = (N, T, heads, hd)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        N, T, H, hd = ctx.geom
        dout = _req(dout, "dout")
        dqkv = torch.empty_like(qkv)
        lib = L.lib()
        nbytes = lib.seld_mha_bwd_workspace(N, T, H)
        wsb = torch.empty((nbytes + 3) // 4, device=qkv.device, dtype=torch.float32)
        L.check(lib.seld_mha_bwd_packed(L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), N, T, H, hd, L.ptr(dqkv),
                                        L.ptr(wsb), nbytes, L.current_stream()), "seld_mha_bwd_packed")
        return dqkv, None


def mha_packed_ok(T, head_dim):
    return bool(L.lib().seld_mha_packed_ok(int(T), int(head_dim)))


def mha_core_packed(qkv, heads):
    return MhaPackedFn.apply(qkv, heads)
